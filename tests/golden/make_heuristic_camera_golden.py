#!/usr/bin/env python3
"""Generator of tests/golden/heuristic_camera_*.npz: the reference's HeuristicCameraAgent (mate/agents/heuristic.py:17-287) playing the
cameras against GreedyTargetAgent, recorded step by step with make_golden.py's machinery -- make_trace(..., policy='greedy',
record_agents=True), whose `GreedyCameraAgent` name is pointed at the heuristic class for the duration of the trace, so the Bernoulli and
sample uniforms are logged as for the Greedy cameras.

Beyond the keys of greedy_*.npz:
    step/hcam_permutations [T][32][Nc]   the permutations the controller drew (its generator's `permutation` is wrapped HERE, in this
                                         process; the reference's files are not touched)
    step/hcam_goal_index [T][Nc]         the state index of every camera's goal, -1 where it has none
    step/hcam_goal [T][Nc][2]            the goal (orientation, viewing angle), NaN where none
    table/state_mesh, table/coord_grid   the reference's tables; table/score_rows [24][756] with table/score_row_index [24]; and
    table/scores_sha256                  of the whole score table's bytes (informative: libm may differ between machines)
Arrays and names only are stored: data, no program text.  A seed is accepted only if the restatement of tests/heuristic_camera_ref.py
reproduces every goal index exactly and every camera action to 1e-9, every decision margin exceeds 1e-9, at least 5 % of the camera-steps
have no goal with both of their branches taken, and (8v8-9) some pick differs from the camera's solo argmax.

    MATE_REFERENCE=<checkout of XuehaiPan/mate> python tests/golden/make_heuristic_camera_golden.py
"""
import hashlib
import os
import sys

import numpy as np

if not hasattr(np, 'bool8'):
    np.bool8 = np.bool_      # (the agent's spelling; gone from NumPy 2)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # mate_amd (its tables, no device)
import make_golden as MG  # noqa: E402  (puts the shim and the reference on sys.path, imports gym and mate)
from heuristic_camera_ref import fixture_inputs, heuristic_cameras  # noqa: E402

from mate.agents.heuristic import HeuristicCameraAgent  # noqa: E402

ROWS = np.linspace(0, 2951, 24).astype(np.int64)      # the recorded rows of the score table: both rims and the interior


def heuristic_camera_fixture(name, config, seed, steps, need_solo_difference=False):
    greedy_class = MG.GreedyCameraAgent
    real_goal = HeuristicCameraAgent.get_joint_goal_state
    calls = []

    def recording_goal(self, camera_states, target_states):
        assert self.index == 0, 'only the controller computes the joint goal'
        drawn = []
        held = self.np_random

        class Draws:
            def __getattr__(_, attr):
                return getattr(held, attr)

            def permutation(_, x):
                out = held.permutation(x)
                drawn.append(np.array(out, dtype=np.int64))
                return out

        self._np_random = Draws()
        try:
            goal = real_goal(self, camera_states, target_states)
        finally:
            self._np_random = held
        tables = (self.state_mesh, self.coord_grid, self.scores)
        calls.append((np.stack(drawn), {c: goal[c] for c in range(self.num_cameras)}, tables))
        return goal

    HeuristicCameraAgent.get_joint_goal_state = recording_goal
    MG.GreedyCameraAgent = HeuristicCameraAgent
    try:
        MG.make_trace(name, config, seed, 'greedy', steps, record_agents=True)
    finally:
        MG.GreedyCameraAgent = greedy_class
        HeuristicCameraAgent.get_joint_goal_state = real_goal
    path = os.path.join(HERE, name + '.npz')
    out = dict(np.load(path))
    T, Nc = len(out['step/done']), int(out['num_cameras'])
    assert len(calls) == T, (len(calls), T)
    mesh, grid, scores = calls[0][2]
    out['step/hcam_permutations'] = np.stack([p for p, _, _ in calls]).astype(np.int8)
    goal = np.full((T, Nc, 2), np.nan)
    index = np.full((T, Nc), -1, dtype=np.int64)
    for s, (_, g, _) in enumerate(calls):
        for c in range(Nc):
            if None not in g[c]:
                goal[s, c] = g[c]
                hit = np.flatnonzero((mesh[:, 0] == g[c][0]) & (mesh[:, 1] == g[c][1]))
                assert len(hit) == 1
                index[s, c] = hit[0]
    out['step/hcam_goal'], out['step/hcam_goal_index'] = goal, index
    out['table/state_mesh'], out['table/coord_grid'] = np.array(mesh), np.array(grid)
    out['table/score_row_index'], out['table/score_rows'] = ROWS, np.array(scores[ROWS])
    out['table/scores_sha256'] = np.str_(hashlib.sha256(np.ascontiguousarray(scores).tobytes()).hexdigest())
    out['policy'] = np.str_('heuristic_camera')
    for key in ('reset/cam_obs', 'reset/tgt_obs', 'reset/state', 'step/target_warehouse_distances', 'step/target_obstacle_view_mask',
                'step/target_target_view_mask', 'step/camera_camera_view_mask'):
        out.pop(key, None)

    from mate_amd.heuristic_tables import heuristic_camera_tables
    tables = heuristic_camera_tables(float(out['static/cam_max_sight_range'][0]), float(out['static/cam_min_viewing_angle'][0]))
    action, got_index, got_goal, info = heuristic_cameras(tables=tables, **fixture_inputs(out))
    worst = float(np.abs(action - out['step/cam_act']).max())
    none = index < 0
    margin = float(info['margin'].min())
    print(f'{name}: {T} steps, goal indices differ at {int((got_index != index).sum())}, |restatement - recorded action| = {worst:.2e}, '
          f'no goal {none.mean():.3f} (kept {int(info["kept"].sum())}, resampled {int(info["resampled"].sum())}), '
          f'picks off the solo argmax {int(info["solo_differs"].sum())}, smallest margin {margin:.2e}')
    assert np.array_equal(got_index, index)
    assert np.array_equal(np.isnan(got_goal), np.isnan(goal)) and np.array_equal(np.nan_to_num(got_goal), np.nan_to_num(goal))
    assert worst < 1e-9, worst
    assert margin > 1e-9, margin
    assert none.mean() >= 0.05 and info['kept'].any() and info['resampled'].any(), name
    assert not need_solo_difference or info['solo_differs'].any(), name
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(f'    {size / 1024:.0f} KiB')
    return out


def main():
    heuristic_camera_fixture('heuristic_camera_4v8-9_s61', 'MATE-4v8-9.yaml', 61, 80)
    heuristic_camera_fixture('heuristic_camera_8v8-9_s62', 'MATE-8v8-9.yaml', 62, 60, need_solo_difference=True)
    for seed in range(63, 93):      # (the first seed that meets every condition: most 2v4-0 episodes keep every camera busy throughout)
        name = f'heuristic_camera_2v4-0_s{seed}'
        try:
            heuristic_camera_fixture(name, 'MATE-2v4-0.yaml', seed, 120)
            break
        except AssertionError as err:
            print(f'    seed {seed} not accepted: {err!r}')
            os.remove(os.path.join(HERE, name + '.npz'))
    else:
        raise SystemExit('no accepted seed for MATE-2v4-0')


if __name__ == '__main__':
    main()
