"""The entity-count edge matrix: scenarios, seeds, batch sizes and step counts shared by tests/test_gpu_shape_edges.py (HIP
engine vs the oracle) and tests/test_shape_edges_cpu.py (the oracle alone: do the targets really run into the circles the
case is about?).  Both take a case from CASES, so the inputs that were counted are the inputs that are compared.

The kernels switch algorithm on thresholds of the entity counts (mate_amd/csrc/engine_kernels.hpp simulate_targets: a target
walks NK = No + Nc circles, obstacles first, then cameras; the collision screen has a ballot form for Nt * NK <= 320 and
NK <= 64 and an LDS form with two 32-bit words per target for everything else; reset_kernels.hpp sorts the occlusion tables
in LDS up to 16 obstacles and in an HBM scratch slice beyond).  Every case stands on one of them.

The geometry: up to 16 cameras in narrow boxes on a 4 x 4 grid (400 apart), up to 64 small obstacles on the 8 x 8 grid whose
cells the cameras are the corners of (200 apart, so a camera's nearest obstacles are 141 away), and every target in a box
around a camera -- where there are fewer targets than cameras, around the LAST ones -- so that 20-unit steps of the random
policy run into that camera's body from the first step on.  Scenarios without cameras put the targets around obstacles,
the last one (circle No - 1) first, with shuffle_entities off so that it is that obstacle.
"""
import collections

import numpy as np

Case = collections.namedtuple('Case', 'shape n steps seed first why')

CASES = [
    # NK = 65: the smallest scenario past 64 circles; camera 0 is circle 64, the first one the two LDS near words cannot name
    Case((1, 2, 64), 48, 40, 4101, 300, 'NK = 65'),
    # every maximum at once: NK = 80 (cameras are circles 64..79), 1536 range pairs, table sort in the HBM scratch, the
    # c * 64 + o camera-obstacle mask bits full
    Case((16, 16, 64), 8, 30, 4102, 17, 'all maxima, NK = 80'),
    # NK = 64 exactly, Nt * NK = 192: inside ballot_screen, its `NK >= 64 ? ~0ull` mask branch
    Case((16, 3, 48), 24, 40, 4103, 5, 'NK = 64 in the ballot screen'),
    # NK = 64 without cameras, Nt * NK = 320 = 64 * kNearWords: the last shape ballot_screen takes
    Case((0, 5, 64), 32, 40, 4104, 0, 'Nt * NK = 320, last ballot shape'),
    # NK = 64 in the LDS form (Nt * NK = 384): circle 63 is bit 31 of the second near word, `1 << 31` on a signed int
    Case((0, 6, 64), 24, 40, 4105, 9000, 'NK = 64 in the LDS screen, bit 31'),
    # one obstacle apart, on both sides of the screen's boundary: Nt * NK = 320 vs 336 (ballot vs LDS form), 16 vs 17 obstacles
    # in the table build (4096-ray sort arrays either way; whether they fit the LDS beside the shape's own slice or go to the
    # HBM scratch is decided per shape, mate_engine.hip layout_reset_lds)
    Case((4, 16, 16), 12, 40, 4106, 64, 'Nt * NK = 320, 16 obstacles'),
    Case((4, 16, 17), 12, 40, 4107, 64, 'Nt * NK = 336, 17 obstacles'),
    # all counts odd: mask fields straddle 32-bit words, row widths with a ragged 16-byte tail
    Case((3, 5, 7), 32, 40, 4108, 123, 'odd counts'),
    # no obstacles; 81 camera pairs (two rounds of (sender, recipient) pairs)
    Case((9, 2, 0), 48, 40, 4109, 1, 'no obstacles, 81 camera pairs'),
]
# the closed-loop step_greedy comparison: the boundary from one to two message rounds (81 camera pairs) and the four-round
# case with Nt = 16 (`(1u << Nt) - 1u`, policy_kernels.hpp)
GREEDY_CASES = [
    Case((9, 2, 0), 24, 40, 4201, 31, 'greedy, two message rounds'),
    Case((16, 16, 9), 8, 30, 4202, 32, 'greedy, four message rounds, Nt = 16'),
]


def case_id(case):
    return '%dv%d-%d' % case.shape


CAMERA_SITES = [(float(x), float(y)) for y in (-600, -200, 200, 600) for x in (-600, -200, 200, 600)]
OBSTACLE_SITES = [(float(x), float(y)) for y in range(-700, 701, 200) for x in range(-700, 701, 200)]
CAMERA_HALF_BOX = 4.0        # cameras: all but fixed
TARGET_HALF_BOX = 58.0       # targets: around a camera body of radius 40 (a target is never placed inside one)
OBSTACLE_HALF_BOX = 25.0
OBSTACLE_RADII = [6.0, 16.0]
LONE_TARGET_HALF_BOX = 30.0  # scenarios without cameras: around an obstacle


def _box(site, half):
    return [site[0] - half, site[0] + half, site[1] - half, site[1] + half]


def scenario(shape):
    """The scenario mapping of an (Nc, Nt, No) case (validated by read_config)."""
    from mate_amd.config import read_config
    nc, nt, no = shape
    base = read_config('MATE-8v8-9.yaml')
    cfg = {k: v for k, v in base.items() if k not in ('camera', 'target', 'obstacle')}
    cfg['name'] = 'MultiAgentTracking(%dv%d, %d)' % shape
    if nc:
        cfg['camera'] = dict(base['camera'], location_random_range=[_box(CAMERA_SITES[c], CAMERA_HALF_BOX) for c in range(nc)])
        # target t around camera nc - 1 - (t mod nc): the last cameras first
        boxes = [_box(CAMERA_SITES[nc - 1 - t % nc], TARGET_HALF_BOX) for t in range(nt)]
    else:
        cfg['shuffle_entities'] = False
        order = [no - 1, no // 2, no // 2 - 1, 0, no - 2, 1]      # circle 63 (bit 31 of the second word), 32, 31, 0, ...
        boxes = [_box(OBSTACLE_SITES[order[t % len(order)]], LONE_TARGET_HALF_BOX) for t in range(nt)]
    cfg['target'] = dict(base['target'], location_random_range=boxes)
    if no:
        cfg['obstacle'] = dict(base['obstacle'], location_random_range=[_box(OBSTACLE_SITES[o], OBSTACLE_HALF_BOX) for o in range(no)],
                               radius_random_range=list(OBSTACLE_RADII))
    return read_config(cfg)


def oracle_batch(O, case, cfg=None):
    """The oracle's batch of a case, reset (its own occlusion tables)."""
    import gpu_util as U
    cfg = cfg or scenario(case.shape)
    batch = O.OracleBatch(U.oracle_proto_from_config(cfg, O), case.n, seed=case.seed, first_env_index=case.first)
    batch.reset(threads=8)
    return batch


def count_events(O, case, batch=None, cfg=None):
    """Steps the oracle alone through the case's random-policy rollout and counts, over (environment, step, target):
    `colliding` -- the oracle reports tgt_colliding; `camera` -- it does and the clamped intended destination (Target.simulate:
    position + the action cut to the target's step size) lies inside a camera's disc; `camera_past_64` -- the same for cameras
    whose index in the walk, No + c, is 64 or more; `obstacle` -- colliding with the destination inside an obstacle's disc."""
    nc, nt, no = case.shape
    cfg = cfg or scenario(case.shape)
    batch = batch or oracle_batch(O, case, cfg)
    cam = cfg.get('camera', {})
    rot, zoom = cam.get('rotation_step', 0.0), cam.get('zooming_step', 0.0)
    step_size = float(cfg['target']['step_size'])
    cam_xy = np.stack([batch.gather('cam_x'), batch.gather('cam_y')], axis=-1) if nc else np.zeros((case.n, 0, 2))
    cam_r = batch.gather('cam_radius') if nc else np.zeros((case.n, 0))
    obs_xy = np.stack([batch.gather('obs_x'), batch.gather('obs_y')], axis=-1) if no else np.zeros((case.n, 0, 2))
    obs_r = batch.gather('obs_radius') if no else np.zeros((case.n, 0))
    past = (no + np.arange(nc)) >= 64
    counts = collections.Counter(colliding=0, camera=0, camera_past_64=0, obstacle=0)
    for _ in range(case.steps):
        pos = np.stack([batch.gather('tgt_x'), batch.gather('tgt_y')], axis=-1)            # [n, Nt, 2]
        limit = batch.gather('tgt_step_size')                                              # [n, Nt]
        ticks = batch.gather('tick')
        act = np.stack([O.random_actions(case.seed, case.first + e, int(ticks[e]), nc, nt, rot, zoom, step_size)[1] for e in range(case.n)]).astype(np.float64)
        norm = np.hypot(act[..., 0], act[..., 1])
        scale = np.where(norm > limit, limit / np.maximum(norm, 1e-300), 1.0)
        dest = pos + act * scale[..., None]
        batch.step(auto_reset=False, threads=8)
        colliding = batch.gather('tgt_colliding') != 0                                     # [n, Nt]
        # the destination restated here is the oracle's: a target that does not collide stands on it (entities.py:668)
        now = np.stack([batch.gather('tgt_x'), batch.gather('tgt_y')], axis=-1)
        assert np.all((np.abs(now - dest).max(axis=-1) <= 1e-6) == ~colliding)
        in_cam = np.hypot(*np.moveaxis(dest[:, :, None, :] - cam_xy[:, None, :, :], -1, 0)) < cam_r[:, None, :]      # [n, Nt, Nc]
        in_obs = np.hypot(*np.moveaxis(dest[:, :, None, :] - obs_xy[:, None, :, :], -1, 0)) < obs_r[:, None, :]
        counts['colliding'] += int(colliding.sum())
        counts['camera'] += int((colliding & in_cam.any(axis=2)).sum())
        counts['camera_past_64'] += int((colliding & in_cam[:, :, past].any(axis=2)).sum())
        counts['obstacle'] += int((colliding & in_obs.any(axis=2)).sum())
    return dict(counts)
