"""The three tables of the Heuristic camera opponent (Engine.set_camera_opponent), in NumPy: what
HeuristicCameraAgent.calculate_scores (mate/agents/heuristic.py:235-287) tabulates, restated from its description.

    state_mesh [756][3]   state s = a * 36 + o: orientation -180 + 10 o, viewing angle linspace(theta_min, 180, 21)[a],
                          sight range Rmax sqrt(theta_min / angle)
    coord_grid [2952][2]  point g = p * 41 + r: radius linspace(0, Rmax, 41)[r] at polar angle -180 + 5 p, Cartesian
    scores [2952][756]    f64: how well a camera in state s holds a target at offset coord_grid[g] -- the product of
                          (distance to the sector's boundary) / (radius of the sector's incircle) and 1 - rho / sight range,
                          zero outside the sector

One set per (round(Rmax, 8), round(theta_min, 8)), as the reference keys them; the engine's library has no generator of its own
(mate_engine_heuristic_camera_tables takes the three arrays)."""
import functools

import numpy as np

__all__ = ['heuristic_camera_tables', 'N_ORIENTATIONS', 'N_ANGLES', 'N_STATES', 'N_RADII', 'N_POLAR', 'N_POINTS', 'N_PERMUTATIONS']

N_ORIENTATIONS, N_ANGLES = 36, 21
N_STATES = N_ORIENTATIONS * N_ANGLES        # 756
N_RADII, N_POLAR = 41, 72
N_POINTS = N_RADII * N_POLAR                # 2952
N_PERMUTATIONS = 32
MAX_VIEWING_ANGLE = 180.0


def _sin_deg(x):
    return np.sin(np.deg2rad(x))


@functools.lru_cache(maxsize=None)
def _tables(max_sight_range, min_viewing_angle):
    orientation = np.tile(np.linspace(-180.0, 180.0, N_ORIENTATIONS, endpoint=False), N_ANGLES)
    angle = np.repeat(np.linspace(min_viewing_angle, MAX_VIEWING_ANGLE, N_ANGLES, endpoint=True), N_ORIENTATIONS)
    sight = max_sight_range * np.sqrt(min_viewing_angle / angle)
    state_mesh = np.stack([orientation, angle, sight], axis=-1)

    rho = np.tile(np.linspace(0.0, max_sight_range, N_RADII, endpoint=True), N_POLAR)
    phi = np.repeat(np.linspace(-180.0, 180.0, N_POLAR, endpoint=False), N_RADII)
    phi_rad = np.deg2rad(phi)
    coord_grid = np.stack([rho * np.cos(phi_rad), rho * np.sin(phi_rad)], axis=-1)

    # [G, S]: every (grid point, state) at once, the operations per element in the order of the per-state loop
    half = (angle / 2.0)[None, :]
    reach = sight[None, :]
    with np.errstate(divide='ignore'):
        incircle = np.where(angle[None, :] < 180.0, reach / (1.0 + 1.0 / _sin_deg(half)), reach / 2.0)
    r = rho[:, None]
    delta = np.abs((phi[:, None] - orientation[None, :] + 180.0) % 360.0 - 180.0)
    inside = (r <= reach) & (delta <= half)
    to_arc = np.minimum(r, reach - r)
    to_side = r * _sin_deg(np.minimum(half - delta, 90.0))
    to_boundary = np.maximum(np.minimum(to_arc, to_side), 0.0)
    scores = np.where(inside, (to_boundary / incircle) * (1.0 - r / reach), 0.0)
    for table in (state_mesh, coord_grid, scores):
        table.setflags(write=False)
    return state_mesh, coord_grid, np.ascontiguousarray(scores)


def heuristic_camera_tables(max_sight_range, min_viewing_angle):
    """(state_mesh [756, 3], coord_grid [2952, 2], scores [2952, 756]) f64, read-only, cached per rounded pair."""
    return _tables(round(float(max_sight_range), 8), round(float(min_viewing_angle), 8))
