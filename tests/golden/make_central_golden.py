#!/usr/bin/env python3
"""Generator of tests/golden/central_*.npz: the rows of the reference trainers' centralised-training wrapper over the reference's own environment
under the trainers' chain

    MultiCamera(GreedyTargetAgent) | MultiTarget(GreedyCameraAgent) -> RelativeCoordinates -> RescaledObservation -> RepeatedRewardIndividualDone
        [-> HierarchicalCamera(multi_selection, frame_skip=1)]

driven on the CPU.  Imports the upstream reference read-only (its checkout is named by the MATE_REFERENCE environment variable) under the `gymshim`
package next to this file.  RLlibMultiAgentAPI and RLlibMultiAgentCentralizedTraining live in `examples.utils`, which needs ray and gym: CentralizedRows
below is a stand-in written here.  Its cyclic arrangement -- teammates from the agent's successor on, `cycled[i + 1 : i + n]`, zeros for the action block
in reset(), the joint action of the step that has just run in step() -- is this file's restatement of examples/utils/wrappers.py:176-251; the state is
mate.normalize_observation(env.state(), env.state_space), the wrapper's default, and the action mask the environment's own action_mask().  HierarchicalCamera
is the reference's class (imported as make_selection_golden.py does).  Arrays and names only are stored: data, no program text.

Per recorded row t (row 0: reset(); a row behind a finished episode: the reset() the trainer calls): the joint observation [n, D], the normalised state [S],
the joint action that led to it ([n, ...]; zeros at a reset row), done, whether it is a reset row, and per agent the wrapper's blocks.  The episode is cut short
(max_episode_steps) so that one recording runs through an episode end and the reset behind it.

    MATE_REFERENCE=<checkout of XuehaiPan/mate> python tests/golden/make_central_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the shim and the reference on sys.path, imports gym and mate)
import make_selection_golden as MS  # noqa: E402  (the MultiBinary shim, examples.hrl.wrappers under a stand-in examples.utils)

mate = MG.mate
if not hasattr(np, 'bool8'):
    np.bool8 = np.bool_


class CentralizedRows:
    """The stand-in for RLlibMultiAgentAPI + RLlibMultiAgentCentralizedTraining over sequences instead of agent-id dictionaries."""

    def __init__(self, env, add_joint_observation=False, add_action_mask=False):
        self.env, self.add_joint_observation, self.add_action_mask = env, add_joint_observation, add_action_mask
        self.n = len(env.observation_space.spaces)

    def state(self):
        return mate.normalize_observation(self.env.state(), self.env.state_space)

    def _rows(self, observations, joint_action):
        n = self.n
        joint_observation = tuple(observations)
        cycled_observation = joint_observation + joint_observation
        cycled_action = tuple(joint_action) + tuple(joint_action)
        state = self.state()
        rows = []
        for i in range(n):
            row = {'obs': observations[i], 'state': state, 'prev_others_joint_action': cycled_action[i + 1:i + n]}
            if self.add_action_mask:
                row['action_mask'] = self.env.action_mask(observations[i])
            if self.add_joint_observation:
                row['others_joint_observation'] = cycled_observation[i + 1:i + n]
            rows.append(row)
        return rows

    def reset(self, zero_action):
        observations = self.env.reset()
        return observations, self._rows(observations, [np.zeros_like(zero_action)] * self.n)

    def step(self, joint_action):
        observations, rewards, dones, infos = self.env.step(joint_action)
        return observations, self._rows(observations, joint_action), dones


def central_fixture(name, config, seed, learner, steps, max_episode_steps, levels=None, hierarchical=False, joint_observation=False):
    base = mate.make('MultiAgentTracking-v0', config=config, reward_type='dense', max_episode_steps=max_episode_steps)
    grid = None
    if learner == 'camera':
        env = mate.MultiCamera(base, target_agent=MG.GreedyTargetAgent(seed=0))
    else:
        if levels:
            base = mate.DiscreteTarget(base, levels=levels)
            grid = np.asarray(base.normalized_action_grid, dtype=np.float64)
        env = mate.MultiTarget(base, camera_agent=MG.GreedyCameraAgent(seed=0))
    env = mate.RepeatedRewardIndividualDone(mate.RescaledObservation(mate.RelativeCoordinates(env)))
    if hierarchical:
        env = MS.import_wrappers().HierarchicalCamera(env, multi_selection=True, frame_skip=1, custom_metrics={})
    env.seed(seed)
    wrapper = CentralizedRows(env, add_joint_observation=joint_observation, add_action_mask=hierarchical)
    n, Nt = wrapper.n, env.num_targets
    rng = np.random.RandomState(seed + 3000)

    def draw_action():
        if hierarchical:
            return (rng.random_sample((n, Nt)) < 0.4).astype(np.int64)
        if levels:
            return rng.randint(0, len(grid), size=n).astype(np.int64)
        high = np.asarray(env.action_space.spaces[0].high, dtype=np.float64)
        return rng.uniform(-1.0, 1.0, size=(n, 2)) * high

    out = {key: [] for key in ('step/obs', 'step/state', 'step/action', 'step/done', 'step/reset', 'row/obs', 'row/state', 'row/prev_others_joint_action',
                               'row/action_mask', 'row/others_joint_observation')}

    def record(observations, rows, action, done, is_reset):
        out['step/obs'].append(np.asarray(observations, dtype=np.float64))
        out['step/state'].append(np.asarray(rows[0]['state'], dtype=np.float64))
        out['step/action'].append(np.asarray(action))
        out['step/done'].append(bool(done))
        out['step/reset'].append(bool(is_reset))
        out['row/obs'].append(np.stack([np.asarray(r['obs'], dtype=np.float64) for r in rows]))
        out['row/state'].append(np.stack([np.asarray(r['state'], dtype=np.float64) for r in rows]))
        out['row/prev_others_joint_action'].append(np.stack([np.asarray(r['prev_others_joint_action']).reshape(-1) for r in rows]))
        if hierarchical:
            out['row/action_mask'].append(np.stack([np.asarray(r['action_mask'], dtype=np.uint8) for r in rows]))
        if joint_observation:
            out['row/others_joint_observation'].append(np.stack([np.asarray(r['others_joint_observation'], dtype=np.float64).reshape(-1) for r in rows]))

    zero = draw_action()[0] * 0
    observations, rows = wrapper.reset(zero)
    record(observations, rows, np.stack([zero] * n), False, True)
    for _ in range(steps):
        action = draw_action()
        observations, rows, dones = wrapper.step(action)
        record(observations, rows, action, all(dones), False)
        if all(dones):
            observations, rows = wrapper.reset(zero)
            record(observations, rows, np.stack([zero] * n), False, True)
    fx = {key: np.asarray(value) for key, value in out.items() if value}
    assert fx['step/done'].sum() == 1 and fx['step/reset'].sum() == 2 and not fx['step/reset'][-1], (fx['step/done'], fx['step/reset'])
    fx.update({
        'config_file': np.str_(config), 'seed': np.int64(seed), 'learner_team': np.str_(learner), 'num_cameras': np.int64(env.num_cameras),
        'num_targets': np.int64(Nt), 'num_obstacles': np.int64(env.num_obstacles), 'max_episode_steps': np.int64(max_episode_steps),
        'joint_observation': np.bool_(joint_observation), 'hierarchical': np.bool_(hierarchical), 'discrete_levels': np.int64(levels or 0),
        'block_names': np.asarray([key[4:] for key in fx if key.startswith('row/')]),
    })
    if grid is not None:
        fx['action_grid'] = grid
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **fx)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith('.npz') and not f.startswith('central_'))
    assert os.path.getsize(path) <= largest, (os.path.getsize(path), largest)
    print(name, len(fx['step/done']), 'rows', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    central_fixture('central_4v8-9_camera_joint', 'MATE-4v8-9.yaml', 71, 'camera', steps=12, max_episode_steps=8, joint_observation=True)
    central_fixture('central_2v4-0_target_discrete', 'MATE-2v4-0.yaml', 72, 'target', steps=12, max_episode_steps=8, levels=5)
    central_fixture('central_4v8-9_hierarchical', 'MATE-4v8-9.yaml', 73, 'camera', steps=12, max_episode_steps=8, hierarchical=True)
