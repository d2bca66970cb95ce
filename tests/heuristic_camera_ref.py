"""NumPy restatement of HeuristicCameraAgent (mate/agents/heuristic.py:17-231) under mate.group_step, batched: the central computation of
the controller (camera 0) and every camera's act().  The reference of tests/test_gpu_heuristic_camera.py's batch test, itself pinned to the
recorded reference by tests/test_heuristic_camera_host.py.  Draws are inputs: the 32 permutations, the Bernoulli and the sample uniforms.

Leading batch axis B everywhere:
    cam_xy [B, Nc, 2]   cam_phi, cam_theta [B, Nc]   tgt_xy [B, Nt, 2]   seen [B, Nc, Nt] camera_target_view_mask the agents act on
    permutations [B, 32, Nc]   prev_action [B, Nc, 2]   binom_u [B, Nc]   sample_u [B, Nc, 2]
    rot, zoom, rmax: the cameras' rotation_step, zooming_step, max_sight_range; tables: (state_mesh, coord_grid, scores)
Returns (action [B, Nc, 2], goal_index [B, Nc] (-1: none), goal [B, Nc, 2] (NaN: none), info); info holds per environment `margin`, the
smallest relative distance of any discrete decision to a tie:
    in range              |norm - Rmax| / Rmax of every (camera, sensed target) pair (the device's norm fuses its multiply-add)
    nearest grid point    (next distinct - first) / next distinct of the distances to the grid (the 72 points of radius 0 coincide)
    pick                  (largest - next distinct) / largest of scores + untracked count, for every pick of every permutation
    winner                against every permutation that gives some camera with targets another state: the gap of the totals over the
                          winner's total, or, the totals equal, the gap of the costs over the winner's cost
(`margins`: the four of them apart, keys 'range', 'nearest', 'pick', 'winner') and `solo_differs` [B, Nc] (the winner's state of a camera with targets is not the argmax of its own scores + bit counts), `resampled`
and `kept` [B, Nc] (the two no-goal branches).
"""
import numpy as np

TINY = 1e-300


def normalize_angle(a):
    return (a + 180.0) % 360.0 - 180.0      # mate/utils.py:155-158


def sensed_order(seen):
    """Insertion order of the controller's target_states: cameras ascending, within a camera the not yet listed targets ascending."""
    order = []
    for row in seen:
        for t in np.flatnonzero(row):
            if t not in order:
                order.append(int(t))
    return order


def _popcount(x):
    x = x.astype(np.uint32)
    count = np.zeros(x.shape, dtype=np.int64)
    for k in range(16):
        count += (x >> k) & 1
    return count


def heuristic_cameras(cam_xy, cam_phi, cam_theta, tgt_xy, seen, permutations, prev_action, binom_u, sample_u, rot, zoom, rmax, tables):
    mesh, grid, scores = tables
    cam_xy, tgt_xy = np.asarray(cam_xy, dtype=np.float64), np.asarray(tgt_xy, dtype=np.float64)
    cam_phi, cam_theta = np.asarray(cam_phi, dtype=np.float64), np.asarray(cam_theta, dtype=np.float64)
    seen = np.asarray(seen).astype(bool)
    permutations = np.asarray(permutations).astype(np.int64)
    B, Nc, Nt = seen.shape
    S = mesh.shape[0]
    P = permutations.shape[1]
    parts = {key: np.full(B, np.inf) for key in ('range', 'nearest', 'pick', 'winner')}

    # in-range pairs and their nearest grid points
    d = tgt_xy[:, None, :, :] - cam_xy[:, :, None, :]                                  # [B, Nc, Nt, 2]
    sensed = seen.any(axis=1)                                                          # [B, Nt]
    norm = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    in_range = sensed[:, None, :] & (norm <= rmax)
    if Nc and Nt:
        parts['range'] = np.where(np.broadcast_to(sensed[:, None, :], norm.shape), np.abs(norm - rmax) / rmax, np.inf).min(axis=(1, 2))
    nearest = np.zeros((B, Nc, Nt), dtype=np.int64)
    bi, ci, ti = np.nonzero(in_range)
    for lo in range(0, len(bi), 512):
        sl = slice(lo, lo + 512)
        e = d[bi[sl], ci[sl], ti[sl]][:, None, :] - grid[None, :, :]
        dist = np.sqrt(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1])
        g = np.argmin(dist, axis=-1)
        nearest[bi[sl], ci[sl], ti[sl]] = g
        first = dist.min(axis=-1)      # (the 72 points of radius 0 coincide: equal distances are no decision, the first index wins)
        second = np.where(dist > first[:, None], dist, np.inf).min(axis=-1)
        np.minimum.at(parts['nearest'], bi[sl], (second - first) / np.maximum(second, TINY))

    # scores_c and bits_c in list order
    acc = np.zeros((B, Nc, S))
    bits = np.zeros((B, Nc, S), dtype=np.int64)
    orders = [sensed_order(seen[b]) for b in range(B)]
    for k in range(max([len(o) for o in orders] + [0])):
        have = np.array([len(o) > k for o in orders])
        t = np.array([o[k] if len(o) > k else 0 for o in orders])
        use = have[:, None] & in_range[np.arange(B), :, t]                             # [B, Nc]
        rows = scores[nearest[np.arange(B), :, t]]                                     # [B, Nc, S]
        acc = np.where(use[..., None], acc + rows, acc)
        bits = np.where(use[..., None] & (rows > 0), bits | (1 << t)[:, None, None], bits)
    counts = in_range.sum(axis=-1)                                                     # [B, Nc]

    # the 32 greedy assignments
    cur = np.zeros((B, P), dtype=np.int64)
    total = np.zeros((B, P))
    cost = np.zeros((B, P))
    indices = np.zeros((B, P, Nc), dtype=np.int64)
    rows_b = np.arange(B)[:, None]
    for j in range(Nc):
        c = permutations[:, :, j]                                                      # [B, P]
        values = acc[rows_b, c] + _popcount(bits[rows_b, c] & ~cur[..., None])         # [B, P, S]
        i = np.argmax(values, axis=-1)
        top = values.max(axis=-1)
        rest = np.where(values < top[..., None], values, -np.inf).max(axis=-1)
        with np.errstate(invalid='ignore', divide='ignore'):
            gap = np.where(np.isfinite(rest), (top - rest) / np.maximum(top, TINY), np.inf)
        parts['pick'] = np.minimum(parts['pick'], gap.min(axis=-1))
        diff_o = np.abs(mesh[i, 0] - cam_phi[rows_b, c]) / rot
        diff_a = np.abs(mesh[i, 1] - cam_theta[rows_b, c]) / zoom
        cost = cost + np.maximum(diff_o, diff_a)
        cur = cur | np.take_along_axis(bits[rows_b, c], i[..., None], axis=-1)[..., 0]
        total = total + np.take_along_axis(acc[rows_b, c], i[..., None], axis=-1)[..., 0]
        indices[:, :, j] = i
    total = total + _popcount(cur)

    goal_index = np.full((B, Nc), -1, dtype=np.int64)
    solo = np.argmax(acc + _popcount(bits), axis=-1)                                   # [B, Nc]
    for b in range(B):
        keys = [(total[b, k], -cost[b, k], tuple(permutations[b, k]), tuple(indices[b, k])) for k in range(P)]
        w = max(range(P), key=lambda k: keys[k])
        state_of = np.zeros((P, Nc), dtype=np.int64)
        state_of[np.arange(P)[:, None], permutations[b]] = indices[b]
        busy = counts[b] > 0
        goal_index[b, busy] = state_of[w, busy]
        for k in range(P):
            if (state_of[k, busy] != state_of[w, busy]).any():
                if total[b, k] != total[b, w]:
                    parts['winner'][b] = min(parts['winner'][b], abs(total[b, w] - total[b, k]) / max(abs(total[b, w]), TINY))
                elif cost[b, k] != cost[b, w]:
                    parts['winner'][b] = min(parts['winner'][b], abs(cost[b, w] - cost[b, k]) / max(abs(cost[b, w]), TINY))
    has = goal_index >= 0
    safe = np.where(has, goal_index, 0)
    goal = np.where(has[..., None], mesh[safe, :2], np.nan)

    limit = np.array([rot, zoom], dtype=np.float64)
    toward = np.stack([normalize_angle(mesh[safe, 0] - cam_phi), mesh[safe, 1] - cam_theta], axis=-1)
    toward = np.clip(toward, -limit, limit)
    binom_u, sample_u = np.asarray(binom_u, dtype=np.float64), np.asarray(sample_u, dtype=np.float64)
    resampled = ~has & (binom_u > 1.0 - 0.1)
    kept = ~has & ~resampled
    sampled = -limit + (2.0 * limit) * sample_u
    action = np.where(has[..., None], toward, np.where(resampled[..., None], sampled, np.asarray(prev_action, dtype=np.float64)))
    margin = np.minimum(np.minimum(parts['range'], parts['nearest']), np.minimum(parts['pick'], parts['winner']))
    return action, goal_index, goal, {'margin': margin, 'margins': parts, 'solo_differs': has & (goal_index != solo), 'resampled': resampled, 'kept': kept,
                                      'counts': counts, 'total': total, 'cost': cost, 'indices': indices}


def fixture_inputs(fx):
    """The recorded inputs of every step of a heuristic_camera_*.npz fixture: the state and the masks the agents of step s acted on are
    those the step before (or the reset) left; prev_action is the action recorded for the step before ((0, 0) at the first)."""
    def before(key):
        return np.concatenate([fx['reset/' + key][None], fx['step/' + key][:-1]], axis=0)
    T = len(fx['step/done'])
    Nc = int(fx['num_cameras'])
    prev = np.concatenate([np.zeros((1, Nc, 2)), fx['step/cam_act'][:-1]], axis=0)
    return dict(cam_xy=np.broadcast_to(fx['static/cam_xy'], (T, Nc, 2)), cam_phi=before('cam_phi'), cam_theta=before('cam_theta'),
                tgt_xy=before('tgt_xy'), seen=before('camera_target_view_mask'), permutations=fx['step/hcam_permutations'], prev_action=prev,
                binom_u=np.nan_to_num(fx['step/agent_cam_binom_u'], nan=0.0), sample_u=np.nan_to_num(fx['step/agent_cam_sample_u'], nan=0.0),
                rot=float(fx['static/cam_rotation_step'][0]), zoom=float(fx['static/cam_zooming_step'][0]),
                rmax=float(fx['static/cam_max_sight_range'][0]))
