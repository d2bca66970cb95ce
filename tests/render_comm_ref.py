"""NumPy side of the communication arrows (csrc/trace_rows.hpp, csrc/render_rows.hpp), on top of tests/render_ref.py, no reference
import, no GPU:

  * `trace_step(remaining, edges, duration)`: RenderCommunication.step's rule for one environment and team;
  * `arrows(scene, remaining, duration)`: the wrapper's callback restated -- the dashed lines of both teams in its order;
  * `display_list(scene, remaining, duration)`: render_ref's list with those lines where the callback prepends them to the one-time list;
  * `rasterise` / `rim`: render_ref's with the dashed-line primitive (coverage in the device's operation order; the rim adds the band's outline and the dash
    switches).

A line is a dict like render_ref's primitives: kind 'line', v [2, 2] (first vertex first), rgba, width (pixels), stipple.
"""
import numpy as np

import render_ref as R

F = R.F
HEAD, OFFSET, STROKE, STIPPLE = 0.05 * R.TERRAIN, 0.01 * R.TERRAIN, 2.5, 0x0F0F
TEAM_RGB = ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0))      # cameras blue, targets red


# ------------------------------------------------------------------ the wrapper's state
def trace_step(remaining, edges, duration):
    """One live step: the countdown, then `duration` wherever a message was delivered since the previous step."""
    out = np.maximum(remaining.astype(np.int64) - 1, 0)
    out[np.asarray(edges) > 0] = duration
    return out.astype(remaining.dtype)


# ------------------------------------------------------------------ the callback's lines
def draw_arrow(start, end, rgba, bidirectional):
    start, end = np.asarray(start, dtype=np.float64), np.asarray(end, dtype=np.float64)
    vec = end - start
    norm = np.sqrt(vec[0] * vec[0] + vec[1] * vec[1])
    if norm == 0.0:
        return []
    vec = vec * max(0.9, (norm - HEAD) / norm)
    vec1 = np.array([0.04 * vec[0] + 0.015 * vec[1], -0.015 * vec[0] + 0.04 * vec[1]])
    vec2 = np.array([0.04 * vec[0] - 0.015 * vec[1], 0.015 * vec[0] + 0.04 * vec[1]])
    vec1 = vec1 * min(1.0, HEAD / np.sqrt(vec1[0] * vec1[0] + vec1[1] * vec1[1]))
    vec2 = vec2 * min(1.0, HEAD / np.sqrt(vec2[0] * vec2[0] + vec2[1] * vec2[1]))
    start, end = end - vec, start + vec
    if bidirectional:
        vert = np.array([-vec[1], vec[0]])
        vert = vert * (OFFSET / np.sqrt(vert[0] * vert[0] + vert[1] * vert[1]))
        start, end = start + vert, end + vert
    segments = [(start, end), (end - vec1, end)] + ([] if bidirectional else [(end - vec2, end)])
    return [{'kind': 'line', 'v': np.array(seg), 'rgba': tuple(rgba), 'width': STROKE, 'stipple': STIPPLE} for seg in segments]


def arrows(scene, remaining, duration):
    """`remaining`: (camera matrix or None, target matrix or None), [sender][recipient].  Cameras first, pairs sender-major."""
    out = []
    for team, (matrix, xy) in enumerate(zip(remaining, (scene['cam_xy'], scene['tgt_xy']))):
        if matrix is None:
            continue
        for s in range(len(xy)):
            for r in range(len(xy)):
                if matrix[s][r] > 0:
                    alpha = min(1.0, 1.2 * int(matrix[s][r]) / duration)
                    out += draw_arrow(xy[s], xy[r], TEAM_RGB[team] + (alpha,), matrix[r][s] > 0)
    return out


def display_list(scene, remaining, duration):
    prims = R.display_list(scene)
    static = 5 + len(np.asarray(scene['obs_xyr']).reshape(-1, 3))      # margin, warehouses, obstacles: viewer.geoms; the callback prepends to what follows
    return prims[:static] + arrows(scene, remaining, duration) + prims[static:]


# ------------------------------------------------------------------ the dashed line
def _line_terms(prim, size):
    """(squared distance to the segment, distance of the clamped projection from the first vertex along the major axis) of every pixel centre."""
    xs, ys = R.centres(size)
    X, Y = xs[None, :], ys[:, None]
    (ax, ay), (bx, by) = prim['v']
    ex, ey = bx - ax, by - ay
    t = np.clip(((X - ax) * ex + (Y - ay) * ey) / (ex * ex + ey * ey), 0.0, 1.0)
    qx, qy = t * ex, t * ey
    ox, oy = X - (ax + qx), Y - (ay + qy)
    along = np.abs(qx) if abs(ex) >= abs(ey) else np.abs(qy)
    return ox * ox + oy * oy, along


def cover_line(prim, size):
    """Within half the width of the segment, and in an on-phase of the stipple: bit (floor(u) mod 16) of the pattern, u in pixel pitches from the FIRST vertex."""
    p = R.pitch_of(size)
    d2, along = _line_terms(prim, size)
    half = prim['width'] / 2.0 * p
    phase = np.floor(along / p).astype(np.int64) & 15
    return (d2 <= half * half) & (((prim['stipple'] >> phase) & 1) == 1)


def cover(prim, size):
    return cover_line(prim, size) if prim['kind'] == 'line' else R.cover(prim, size)


def rasterise(prims, size):
    image = np.ones((size, size, 3), dtype=F)
    for prim in prims:
        R.blend(image, cover(prim, size), prim['rgba'])
    return R.quantise(image)


def rim(prims, size, eps=1e-6):
    """render_ref.rim, and for a line the pixels within `eps` world units of its band's outline or of a dash switch inside the band."""
    out = R.rim([p for p in prims if p['kind'] != 'line'], size, eps)
    p = R.pitch_of(size)
    for prim in prims:
        if prim['kind'] != 'line':
            continue
        d2, along = _line_terms(prim, size)
        half = prim['width'] / 2.0 * p
        dist = np.sqrt(d2)
        u = along / p
        k = np.round(u / 4.0)
        switch = (k >= 1.0) & (np.abs(u - 4.0 * k) * p <= eps)      # (0x0F0F changes phase at every multiple of 4; u = 0 is the first vertex's cap, no switch)
        out |= (np.abs(dist - half) <= eps) | ((dist <= half + eps) & switch)
    return out


# ------------------------------------------------------------------ recordings (tests/golden/render_comm_*.npz)
# name: (seed, steps, duration, wrapper, tweak) -- what tests/golden/make_render_comm_golden.py ran.  The Greedy targets talk only when a warehouse runs empty:
# the scenes that want red arrows start from few cargoes
RECIPES = {'4v8-9_a': (3, 12, 20, None, None), '4v8-9_b': (3, 45, 20, None, None), '8v8-9': (5, 30, 20, None, None), 'duration3': (7, 59, 3, None, 'few_cargoes'),
           'nocamera': (9, 75, 20, 'no_camera_communication', 'few_cargoes')}
SCENES = tuple(RECIPES)
CONFIGS = {'4v8-9_a': 'MATE-4v8-9.yaml', '4v8-9_b': 'MATE-4v8-9.yaml', '8v8-9': 'MATE-8v8-9.yaml', 'duration3': 'MATE-4v8-9.yaml', 'nocamera': 'MATE-4v8-9.yaml'}
SIZES = {name: (64, 72, 200) + ((800,) if name == '4v8-9_b' else ()) for name in SCENES}      # the sizes the device tests draw a scene at


def load_recording(path):
    """(recorded display list, scene for display_list, the whole fixture) of one tests/golden/render_comm_*.npz."""
    fx = dict(np.load(path, allow_pickle=False))
    starts, names = fx['list/start'], ('polygon', 'polyline', 'line')
    prims = [{'kind': names[int(fx['list/kind'][i])], 'v': fx['list/vertices'][starts[i]:starts[i + 1]].copy(), 'rgba': tuple(float(x) for x in fx['list/rgba'][i]),
              'width': float(fx['list/width'][i]), 'stipple': int(fx['list/stipple'][i])} for i in range(len(starts) - 1)]
    scene = {name: fx['state/' + name] for name in R.STATE_FIELDS}
    scene['cam_radius'], scene['cam_area'] = float(fx['cam_radius']), float(fx['cam_area'])
    scene['knots'] = [(fx['knots/phis'][c, :n].copy(), fx['knots/rhos'][c, :n].copy()) for c, n in enumerate(fx['knots/count'])]
    return prims, scene, fx
