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

Case = collections.namedtuple('Case', 'shape n steps seed first why target_box', defaults=(None,))

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
# The attached launches (selection_kernel, reward_rows_kernel, fragment_rows_kernel, heuristic_drift_kernel, state_rows_kernel) read
# camera_target_view_mask from bit 0 of the mask words: camera c's row is bits c * Nt .. c * Nt + Nt - 1, so with Nt in {1, 2, 4, 8, 16}
# -- every shipped scenario -- no row crosses a 32-bit word.  These cases have rows that do (straddling_rows), with every target in a
# central box `target_box` so that the rows on both sides of the boundary fill (tests/test_shape_edges_cpu.py counts it), and the counts
# the state rows' loops divide by at zero.  `steps`: the random-policy steps of the CPU count.
ATTACHED_CASES = [
    # the smallest straddle: 35 view bits, camera 6's row is bits 30..34; S = 181 is odd and 41 is odd, so the state rows of the partial
    # last tile end off a 16-byte boundary for f32 and f64 rows alike (40 environments would end on one: 8 * 181 * 4 = 362 * 16)
    Case((7, 5, 3), 41, 30, 4301, 7, '35 view bits, row 6 straddles', 300.0),
    # 240 bits in 8 words, seven straddling rows (cameras 2, 4, ..., 14), row 14 ends in the last word (the v.count guard); all sixteen
    # lanes of a group are cameras (the SharedFieldOfView butterfly over width 16); a full tile and a half one
    Case((16, 15, 3), 24, 30, 4301, 7, '240 view bits, seven straddling rows', 500.0),
    # straddle at camera 4 (bits 28..34), no obstacles
    Case((5, 7, 0), 40, 30, 4301, 7, 'row 4 straddles, no obstacles', 300.0),
    # the maxima that fit with policies (the shape of GREEDY_CASES): `(1u << Nt) - 1u` at 16, cam_xy[..][32] full, NJ = 41
    Case((16, 16, 9), 20, 30, 4301, 7, 'sixteen by sixteen with policies', 300.0),
    # no cameras: the geometry of CASES
    Case((0, 5, 64), 33, 30, 4301, 7, 'no cameras'),
    # state rows only: S = 621, a tile of E = 4 environments
    Case((16, 16, 64), 8, 30, 4301, 7, 'state rows of all maxima, E = 4'),
]


def case_id(case):
    return '%dv%d-%d' % case.shape


def attached_case(name):
    """The case of ATTACHED_CASES with that id ('7v5-3')."""
    return {case_id(c): c for c in ATTACHED_CASES}[name]


def straddling_rows(nc, nt):
    """{camera: bits of its camera_target_view_mask row in the lower word} for the rows that cross a 32-bit word boundary (the row
    of camera c is bits c * nt .. c * nt + nt - 1 from bit 0: mate_engine_layout.bit_camera_target = 0)."""
    return {c: 32 - c * nt % 32 for c in range(nc) if c * nt // 32 != (c * nt + nt - 1) // 32}


def straddling_frames(view):
    """{camera: frames} over a [..., Nc, Nt] boolean camera_target_view_mask: the frames in which a straddling row has a seen target
    on EACH side of its word boundary at once -- where a row read from one word only differs from the row."""
    view = np.asarray(view).astype(bool)
    nc, nt = view.shape[-2:]
    return {c: int((view[..., c, :low].any(axis=-1) & view[..., c, low:].any(axis=-1)).sum()) for c, low in straddling_rows(nc, nt).items()}


CAMERA_SITES = [(float(x), float(y)) for y in (-600, -200, 200, 600) for x in (-600, -200, 200, 600)]
OBSTACLE_SITES = [(float(x), float(y)) for y in range(-700, 701, 200) for x in range(-700, 701, 200)]
CAMERA_HALF_BOX = 4.0        # cameras: all but fixed
TARGET_HALF_BOX = 58.0       # targets: around a camera body of radius 40 (a target is never placed inside one)
OBSTACLE_HALF_BOX = 25.0
OBSTACLE_RADII = [6.0, 16.0]
LONE_TARGET_HALF_BOX = 30.0  # scenarios without cameras: around an obstacle


def _box(site, half):
    return [site[0] - half, site[0] + half, site[1] - half, site[1] + half]


def scenario(shape, target_box=None):
    """The scenario mapping of an (Nc, Nt, No) case (validated by read_config).  `target_box` = h: every target in the central box
    [-h, h]^2 instead of beside a camera body (most (camera, target) pairs are never seen from there)."""
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
    if target_box is not None:
        boxes = [_box((0.0, 0.0), float(target_box)) for _ in range(nt)]
    cfg['target'] = dict(base['target'], location_random_range=boxes)
    if no:
        cfg['obstacle'] = dict(base['obstacle'], location_random_range=[_box(OBSTACLE_SITES[o], OBSTACLE_HALF_BOX) for o in range(no)],
                               radius_random_range=list(OBSTACLE_RADII))
    return read_config(cfg)


def case_scenario(case):
    return scenario(case.shape, case.target_box)


def oracle_batch(O, case, cfg=None):
    """The oracle's batch of a case, reset (its own occlusion tables)."""
    import gpu_util as U
    cfg = cfg or case_scenario(case)
    batch = O.OracleBatch(U.oracle_proto_from_config(cfg, O), case.n, seed=case.seed, first_env_index=case.first)
    batch.reset(threads=8)
    return batch


def count_events(O, case, batch=None, cfg=None):
    """Steps the oracle alone through the case's random-policy rollout and counts, over (environment, step, target):
    `colliding` -- the oracle reports tgt_colliding; `camera` -- it does and the clamped intended destination (Target.simulate:
    position + the action cut to the target's step size) lies inside a camera's disc; `camera_past_64` -- the same for cameras
    whose index in the walk, No + c, is 64 or more; `obstacle` -- colliding with the destination inside an obstacle's disc."""
    nc, nt, no = case.shape
    cfg = cfg or case_scenario(case)
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


def count_straddling_frames(O, case):
    """{camera: frames} of straddling_frames over the (environment, step) frames of the case's random-policy rollout on the oracle alone."""
    batch = oracle_batch(O, case)
    nc, nt, _ = case.shape
    total = collections.Counter({c: 0 for c in straddling_rows(nc, nt)})
    for _ in range(case.steps):
        batch.step(auto_reset=False, threads=8)
        total.update(straddling_frames(batch.gather('camera_target_view_mask').reshape(case.n, nc, nt) != 0))
    return dict(total)
