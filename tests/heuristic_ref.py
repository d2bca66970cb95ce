"""NumPy restatement of HeuristicTargetAgent's post-processing of the Greedy target action (mate/agents/heuristic.py:298-337), batched:
the reference for the batch test of tests/test_gpu_heuristic.py, itself pinned to the recorded reference by tests/test_heuristic_host.py.

Every array carries leading batch axes B (any shape, possibly none):
    greedy [B, Nt, 2]   GreedyTargetAgent.act's return value          tgt_xy [B, Nt, 2]    step_size [B, Nt] (or broadcastable)
    cam_xy [B, Nc, 2]   cam_phi, cam_theta, cam_sight [B, Nc]          sensed [B, Nt, Nc]   target_camera_view_mask the agents act on
Returns (final [B, Nt, 2], info): info holds, per target, `candidates` (int), `drifted` (the action changed branch: dot >= 0 with a
candidate), `rejected` (a candidate, dot < 0), `clipped` (a component of action + drift left +-step_size) and `margin`, the smallest
relative distance of any branch condition the target evaluated to equality (inf where none was evaluated):
    norm <= 1.2 sight            |norm - 1.2 sight| / (1.2 sight)
    angle_diff <= 1.2 half       |angle_diff - 1.2 half| / (1.2 half), and the wrap of normalize_angle at +-180: its distance / 360
    the first minimum            (second - best) / best of the relative distances to the incentres
    drift_size > cap             |drift_size - cap| / cap
    dot >= 0                     |dot| / (|action| |drift|)
The comparisons are the reference's: the angle test compares the SIGNED difference (heuristic.py:308-311).
"""
import numpy as np


def normalize_angle(a):
    return (a + 180.0) % 360.0 - 180.0      # mate/utils.py:155-158


def heuristic_drift(greedy, tgt_xy, step_size, cam_xy, cam_phi, cam_theta, cam_sight, sensed, noise_scale=0.5):
    greedy, tgt_xy = np.asarray(greedy, dtype=np.float64), np.asarray(tgt_xy, dtype=np.float64)
    cam_xy = np.asarray(cam_xy, dtype=np.float64)
    sensed = np.asarray(sensed).astype(bool)
    Nt, Nc = sensed.shape[-2], sensed.shape[-1]
    step_size = np.broadcast_to(np.asarray(step_size, dtype=np.float64), greedy.shape[:-1])
    phi = np.asarray(cam_phi, dtype=np.float64)[..., None, :]            # [B, 1, Nc]
    theta = np.asarray(cam_theta, dtype=np.float64)[..., None, :]
    sight = np.asarray(cam_sight, dtype=np.float64)[..., None, :]
    info_shape = greedy.shape[:-1]
    if Nc == 0:
        zeros = np.zeros(info_shape, dtype=bool)
        return greedy.copy(), {'candidates': np.zeros(info_shape, dtype=np.int64), 'drifted': zeros, 'rejected': zeros.copy(),
                               'clipped': zeros.copy(), 'margin': np.full(info_shape, np.inf)}
    with np.errstate(divide='ignore', invalid='ignore'):
        direction = tgt_xy[..., :, None, :] - cam_xy[..., None, :, :]      # [B, Nt, Nc, 2]
        norm = np.sqrt(direction[..., 0] * direction[..., 0] + direction[..., 1] * direction[..., 1])
        half = theta / 2.0
        raw = np.degrees(np.arctan2(direction[..., 1], direction[..., 0])) - phi
        angle_diff = normalize_angle(raw)
        in_range = sensed & (norm <= 1.2 * sight)
        candidate = in_range & (angle_diff <= 1.2 * half)
        margin = np.full(sensed.shape, np.inf)
        margin = np.where(sensed, np.abs(norm - 1.2 * sight) / (1.2 * sight), margin)
        wrap = (raw + 180.0) % 360.0
        angle_margin = np.minimum(np.abs(angle_diff - 1.2 * half) / (1.2 * half), np.minimum(wrap, 360.0 - wrap) / 360.0)
        margin = np.where(in_range, np.minimum(margin, angle_margin), margin).min(axis=-1)

        reach = sight / (1.0 + np.sin(np.radians(np.minimum(half, 90.0))))
        centre = cam_xy[..., None, :, :] + reach[..., None] * np.stack([np.cos(np.radians(phi)), np.sin(np.radians(phi))], axis=-1)
        inner = sight - reach
        away = tgt_xy[..., :, None, :] - centre                             # [B, Nt, Nc, 2]
        rel = np.sqrt(away[..., 0] * away[..., 0] + away[..., 1] * away[..., 1]) / inner
        rel = np.where(candidate, rel, np.inf)
        best = np.argmin(rel, axis=-1)                                      # the first minimum, in camera order
        n_candidates = candidate.sum(axis=-1)
        has = n_candidates > 0
        ordered = np.sort(rel, axis=-1)
        if Nc > 1:
            tie = np.where(n_candidates > 1, (ordered[..., 1] - ordered[..., 0]) / ordered[..., 0], np.inf)
            margin = np.where(has, np.minimum(margin, tie), margin)
        drift = np.take_along_axis(away, best[..., None, None], axis=-2)[..., 0, :]      # [B, Nt, 2]
        size = np.sqrt(drift[..., 0] * drift[..., 0] + drift[..., 1] * drift[..., 1])
        cap = step_size * noise_scale
        margin = np.where(has, np.minimum(margin, np.abs(size - cap) / cap), margin)
        scale = np.where(size > cap, cap / size, 1.0)
        drift = drift * scale[..., None]
        dot = greedy[..., 0] * drift[..., 0] + greedy[..., 1] * drift[..., 1]
        lengths = np.sqrt((greedy * greedy).sum(-1)) * np.sqrt((drift * drift).sum(-1))
        margin = np.where(has, np.minimum(margin, np.where(lengths > 0.0, np.abs(dot) / lengths, 0.0)), margin)
        moved = greedy + drift
        drifted = has & (dot >= 0.0)
        final = np.where(drifted[..., None], np.clip(moved, -step_size[..., None], step_size[..., None]), greedy)
        clipped = drifted & (np.abs(moved) > step_size[..., None]).any(axis=-1)
    return final, {'candidates': n_candidates, 'drifted': drifted, 'rejected': has & ~drifted, 'clipped': clipped, 'margin': margin}


def fixture_inputs(fx):
    """The recorded inputs of every step of a heuristic_*.npz fixture: the state and the masks the agents of step s acted on are
    those the step before (or the reset) left.  Returns the keyword arguments of heuristic_drift with a leading [T] axis."""
    def before(key):
        return np.concatenate([fx['reset/' + key][None], fx['step/' + key][:-1]], axis=0)
    T = len(fx['step/done'])
    return dict(greedy=fx['step/tgt_act_greedy'], tgt_xy=before('tgt_xy'), step_size=np.broadcast_to(fx['static/tgt_step_size'], (T,) + fx['static/tgt_step_size'].shape),
                cam_xy=np.broadcast_to(fx['static/cam_xy'], (T,) + fx['static/cam_xy'].shape), cam_phi=before('cam_phi'), cam_theta=before('cam_theta'),
                cam_sight=before('cam_sight'), sensed=before('target_camera_view_mask'))
