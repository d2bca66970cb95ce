"""NumPy restatement of what the reference's MoreTrainingInformation wrapper adds to the agents' infos (wrappers/more_training_information.py:42-98
over environment.py:1271-1324), in the column order of csrc/info_rows.hpp: from target positions, goals, the colliding flags, the cargo arrays, the two
view masks and the goals / episode of the previous step to the camera rows [..., Nc, 2], the target rows [..., Nt, 9] and the cargo rows [..., 24].
tests/test_info_rows_host.py holds it to every recorded reference trace; tests/test_gpu_info_rows.py holds info_rows_kernel to it."""
import numpy as np

WAREHOUSES = np.array([[925.0, 925.0], [-925.0, 925.0], [-925.0, -925.0], [925.0, -925.0]])      # constants.py:70-72
WAREHOUSE_RADIUS, NO_GOAL_DISTANCE = 75.0, 1000.0                                                   # TERRAIN_WIDTH / 2
CAMERA_COLUMNS, TARGET_COLUMNS, CARGO_COLUMNS = 2, 9, 24


def warehouse_distances(xy):
    """[..., Nt, 4]: max(|location - WAREHOUSES[w]| - 75, 0); the norm of a 2-vector as NumPy takes it: dx dx + dy dy, the root."""
    d = np.asarray(xy, dtype=np.float64)[..., None, :] - WAREHOUSES
    return np.maximum(np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) - WAREHOUSE_RADIUS, 0.0)


def target_dones(goals, previous_goals, same_episode=True):
    """environment.py:1320-1322 -- the goal differs from the goal before this step and that goal was >= 0; nothing in a step of another episode."""
    goals, previous_goals = np.asarray(goals), np.asarray(previous_goals)
    return (goals != previous_goals) & (previous_goals >= 0) & np.asarray(same_episode, dtype=bool)[..., None]


def rows(xy, goals, colliding, remaining_cargoes, awaiting_cargo_counts, camera_target_view=None, target_camera_view=None, previous_goals=None,
         same_episode=True):
    """(camera rows or None without masks' camera axis, target rows, cargo rows), f64.  `camera_target_view` [..., Nc, Nt] /
    `target_camera_view` [..., Nt, Nc]: None leaves NaN in the three mask columns; `previous_goals` None: individual_done is NaN."""
    xy, goals = np.asarray(xy, dtype=np.float64), np.asarray(goals).astype(np.int64)
    lead, nt = goals.shape[:-1], goals.shape[-1]
    wd = warehouse_distances(xy)
    target = np.full(lead + (nt, TARGET_COLUMNS), np.nan)
    target[..., 0] = goals
    target[..., 1] = np.where(goals >= 0, np.take_along_axis(wd, np.maximum(goals, 0)[..., None], axis=-1)[..., 0], NO_GOAL_DISTANCE)
    target[..., 2:6] = wd
    if previous_goals is not None:
        target[..., 6] = target_dones(goals, np.asarray(previous_goals).astype(np.int64), same_episode)
    target[..., 8] = np.asarray(colliding) != 0
    camera = None
    if camera_target_view is not None:
        ct, tc = np.asarray(camera_target_view) != 0, np.asarray(target_camera_view) != 0
        target[..., 7] = ct.any(axis=-2)
        camera = np.stack([ct.sum(axis=-1).astype(np.float64), tc.any(axis=-2).astype(np.float64)], axis=-1)
    remaining = np.asarray(remaining_cargoes, dtype=np.float64).reshape(lead + (4, 4))
    cargo = np.concatenate([remaining.sum(axis=-1), np.asarray(awaiting_cargo_counts, dtype=np.float64).reshape(lead + (4,)), remaining.reshape(lead + (16,))], axis=-1)
    return camera, target, cargo


def rows_of_engine(sd, masks=None, previous_goals=None, same_episode=True):
    """rows() on Engine.state_dict() and Engine.unpack_masks()."""
    xy = np.stack([sd['tgt_x'], sd['tgt_y']], axis=-1)
    ct = tc = None
    if masks is not None:
        n, nt = np.asarray(sd['tgt_goals']).shape
        ct = np.asarray(masks['camera_target_view_mask']).reshape(n, -1, nt)
        tc = np.asarray(masks['target_camera_view_mask']).reshape(n, nt, -1)
    return rows(xy, sd['tgt_goals'], sd['tgt_colliding'], sd['remaining_cargoes'], sd['awaiting_cargo_counts'], ct, tc, previous_goals, same_episode)


class Model:
    """The attached launch's state across calls: the snapshot of goals and episode numbers, and the rows as the launch leaves them --
    an environment whose scalar record of the described frame says done = 2 keeps rows and snapshot."""

    def __init__(self, sd, nc):
        n, nt = np.asarray(sd['tgt_goals']).shape
        self.camera = np.zeros((n, nc, CAMERA_COLUMNS))
        self.target = np.zeros((n, nt, TARGET_COLUMNS))
        self.cargo = np.zeros((n, CARGO_COLUMNS))
        self.snapshot(sd)

    def snapshot(self, sd, envs=None):
        """Behind a reset, a restart or an import (of the environments `envs` [n] bool; default all): the snapshot-only launch."""
        goals, episode = np.asarray(sd['tgt_goals']).astype(np.int64), np.asarray(sd['episode']).astype(np.int64).reshape(-1)
        if envs is None:
            self.goals, self.episode = goals.copy(), episode.copy()
        else:
            self.goals[envs], self.episode[envs] = goals[envs], episode[envs]

    def step(self, sd, masks, done_column, frames=1):
        """Behind a stepping call of `frames` frames whose last frame's scalar column 2 is `done_column`; `sd`, `masks`: the state the
        launch saw (ahead of any restart)."""
        episode = np.asarray(sd['episode']).astype(np.int64).reshape(-1)
        camera, target, cargo = rows_of_engine(sd, masks, self.goals, episode == self.episode)
        if frames > 1:
            target[..., 6] = np.nan
        ran = np.asarray(done_column) != 2
        if camera is not None and camera.shape[-2]:
            self.camera[ran] = camera[ran]
        self.target[ran], self.cargo[ran] = target[ran], cargo[ran]
        self.snapshot(sd, ran)
        return ran
