#!/usr/bin/env python3
"""Generator of tests/golden/selection_*.npz: the reference's HierarchicalCamera wrapper (examples/hrl/wrappers.py) over
MultiCamera(GreedyTargetAgent(seed=0)), recorded frame by frame under the recording RNG proxies of make_golden.py.

Imports the upstream reference read-only (its checkout is named by the MATE_REFERENCE environment variable) under the `gymshim`
package next to this file.  `examples.hrl.wrappers` imports `examples.utils`, which needs ray: the `examples` / `examples.hrl`
packages are entered into sys.modules as bare namespaces (their __init__ files import every trainer) and `examples.utils` is a
stand-in written here -- CustomMetricCallback.DEFAULT_CUSTOM_METRICS = {} and a MetricCollector (sum / mean / last per key or key
pattern).  Arrays and names only are stored: data, no program text.

Per frame: every random draw of the environment and of the greedy targets (the tapes), the selection, the executor's joint action,
the cameras' view masks before and after, rewards, done, the wrapper's four metrics, the state; per fragment (learner step): the
wrapper's returned rewards, its collected infos, the executed frame count and action_mask() of every returned observation.

    MATE_REFERENCE=<checkout of XuehaiPan/mate> python tests/golden/make_selection_golden.py
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the shim and the reference on sys.path, imports gym and mate)

gym, mate = MG.gym, MG.mate
if not hasattr(np, 'bool8'):
    np.bool8 = np.bool_

if not hasattr(gym.spaces, 'MultiBinary'):      # (the shim has no MultiBinary; the wrapper only constructs it: action_mask_space)
    class MultiBinary:
        def __init__(self, n):
            self.n = int(n)

        def contains(self, x):
            x = np.asarray(x)
            return x.shape == (self.n,) and bool(np.isin(x, (0, 1)).all())

    gym.spaces.MultiBinary = MultiBinary

METRICS = ('num_selected_targets', 'num_valid_selected_targets', 'num_invalid_selected_targets', 'invalid_target_selection_rate')


class MetricCollector:
    """{key or compiled pattern: 'sum' | 'mean' | 'last'} over the infos added since construction."""

    def __init__(self, info_keys):
        self.info_keys, self.values = dict(info_keys), {}

    def _how(self, key):
        for pattern, how in self.info_keys.items():
            if (pattern == key) if isinstance(pattern, str) else bool(pattern.match(key)):
                return how
        return None

    def add(self, info):
        for key, value in info.items():
            if isinstance(key, str) and self._how(key) is not None:
                self.values.setdefault(key, []).append(value)

    def collect(self):
        reduce = {'sum': np.sum, 'mean': np.mean, 'last': lambda v: v[-1]}
        return {key: reduce[self._how(key)](values) for key, values in self.values.items()}


def import_wrappers():
    root = os.path.join(os.environ['MATE_REFERENCE'], 'examples')
    for name, path in (('examples', root), ('examples.hrl', os.path.join(root, 'hrl'))):
        module = types.ModuleType(name)
        module.__path__ = [path]
        sys.modules[name] = module
    utils = types.ModuleType('examples.utils')
    utils.CustomMetricCallback = type('CustomMetricCallback', (), {'DEFAULT_CUSTOM_METRICS': {}})
    utils.MetricCollector = MetricCollector
    sys.modules['examples.utils'] = utils
    return importlib.import_module('examples.hrl.wrappers')


def selection_fixture(name, config, seed, multi, frame_skip, learner_steps, shaping=None, overrides=None):
    import mate.wrappers.single_team as single_team
    W = import_wrappers()
    base = mate.make('MultiAgentTracking-v0', config=config, reward_type='dense', **(overrides or {}))
    multi_camera = mate.MultiCamera(base, target_agent=MG.GreedyTargetAgent(seed=0))
    inner = mate.RepeatedRewardIndividualDone(multi_camera)      # (rewards and dones per camera: what the shaper and the wrapper's all(dones) need)
    if shaping is not None:
        inner = mate.AuxiliaryCameraRewards(inner, coefficients=shaping[0], reduction=shaping[1])
    env = W.HierarchicalCamera(inner, multi_selection=multi, frame_skip=frame_skip, custom_metrics={})
    env.seed(seed)
    tgt_agents = multi_camera.opponent_agents_ordered
    gym.spaces.Box.sample = MG._recording_box_sample
    for agent in tgt_agents:
        agent._np_random = MG.AgentRNG(agent.np_random, MG.AGENT_LOG, None)
    MG.AGENT_LOG.clear()
    opponent_actions, executor_actions = [], []
    real_group_step = single_team.group_step
    real_joint_executor = env.joint_executor

    def recording_group_step(env_, agents, observation, infos=None, **kwargs):
        action = real_group_step(env_, agents, observation, infos, **kwargs)
        opponent_actions.append(np.asarray(action, dtype=np.float64))
        return action

    def recording_joint_executor(joint_action, joint_observation):
        actions = real_joint_executor(joint_action, joint_observation)
        executor_actions.append(np.asarray(actions, dtype=np.float64))
        return actions

    single_team.group_step = recording_group_step
    env.joint_executor = recording_joint_executor
    try:
        observations = env.reset()
        for agent in tgt_agents:
            agent._np_random._who = ('tgt', agent.index)
        reset_draws = MG.drain_agent_log([], tgt_agents)
        log = []
        MG.install_proxies(base, log)
        Nc, Nt, No = base.num_cameras, base.num_targets, base.num_obstacles
        out = {
            'config_file': np.str_(config), 'seed': np.int64(seed), 'policy': np.str_('selection'), 'learner_team': np.str_('camera'),
            'num_cameras': np.int64(Nc), 'num_targets': np.int64(Nt), 'num_obstacles': np.int64(No),
            'transmittance': np.float64(base.obstacle_transmittance), 'max_episode_steps': np.int64(base.max_episode_steps),
            'sparse_reward': np.bool_(base._sparse_reward), 'freight_scale': np.float64(base.freight_scale),
            'bounty_scale': np.float64(base.bounty_scale), 'reward_scale': np.float64(base.reward_scale),
            'max_target_team_episode_reward': np.float64(base.max_target_team_episode_reward),
            'target_step_size': np.float64(base.target_step_size),
            'frame_skip': np.int64(frame_skip), 'multi_selection': np.bool_(multi),
            'camera_min_viewing_angle': np.float64(base.cameras[0].min_viewing_angle), 'camera_max_sight_range': np.float64(base.cameras[0].max_sight_range),
            'camera_rotation_step': np.float64(base.cameras[0].rotation_step), 'camera_zooming_step': np.float64(base.cameras[0].zooming_step),
            'camera_area_product': np.float64(base.cameras[0].area_product),
            'agent/tgt_reset_sample_u': reset_draws['tgt_sample_u'],
            'metric_names': np.asarray(METRICS),
        }
        if shaping is not None:
            out['aux_keys'] = np.asarray(list(shaping[0].keys()))
            out['aux_coefficients'] = np.asarray(list(shaping[0].values()), dtype=np.float64)
            out['aux_reduction'] = np.str_(shaping[1])
        for k, v in MG.snapshot_static(base).items():
            out['static/' + k] = v
        for k, v in MG.snapshot_dynamic(base).items():
            out['reset/' + k] = v
        out['reset/action_mask'] = np.stack([env.action_mask(o) for o in observations]).astype(np.uint8)
        per_step, per_skip = {}, {}

        def push(store, key, value):
            store.setdefault(key, []).append(np.asarray(value))

        rng = np.random.RandomState(seed + 2000)
        mask_slice = env.target_view_mask_slice
        real_env_step = inner.step
        frames_of_fragment = []

        def recording_inner_step(action):      # one FRAME: what the wrapper's loop sees around env.step
            log.clear()
            view_before = np.stack([o[mask_slice] for o in env_last_obs[0]]).astype(bool)
            cams = np.asarray([[c.location[0], c.location[1], c.orientation, c.viewing_angle, c.sight_range] for c in base.cameras], dtype=np.float64)
            tgts = np.asarray([t.location for t in base.targets], dtype=np.float64)
            result = real_env_step(action)
            obs, rewards, dones, infos = result
            tape_ct, _, goal_u, goal_k, goal_j = MG.drain_log(base, log)
            for k, v in MG.drain_agent_log([], tgt_agents).items():
                if k.startswith('tgt_'):
                    push(per_step, 'agent_' + k, v)
            push(per_step, 'executor_act', executor_actions.pop().reshape(Nc, 2))
            push(per_step, 'tgt_act', opponent_actions.pop().reshape(Nt, 2))
            assert not opponent_actions and not executor_actions
            push(per_step, 'selection_bits', current['bits'])
            push(per_step, 'view_before', view_before)
            push(per_step, 'view_after', np.stack([o[mask_slice] for o in obs]).astype(bool))
            push(per_step, 'cam_before', cams)
            push(per_step, 'tgt_xy_before', tgts)
            push(per_step, 'tape_ct', tape_ct)
            push(per_step, 'goal_u', goal_u)
            push(per_step, 'goal_k', goal_k)
            push(per_step, 'goal_j', goal_j)
            push(per_step, 'shaped_reward_cam', np.asarray(rewards, dtype=np.float64))
            if shaping is not None:      # (the shaper keeps the environment's own reward under 'raw_reward'; without one the rewards ARE raw)
                assert 'raw_reward' in infos[0], sorted(infos[0])
            push(per_step, 'reward_cam', infos[0]['raw_reward'] if shaping is not None else rewards[0])
            push(per_step, 'info_coverage_rate', infos[0]['coverage_rate'])
            push(per_step, 'done', bool(all(dones)))
            push(per_step, 'learner_step', current['ls'])
            for k, v in MG.snapshot_dynamic(base).items():
                push(per_step, k, v)
            env_last_obs[0] = obs
            frames_of_fragment.append(infos)
            return result

        inner.step = recording_inner_step
        env_last_obs = [observations]
        current = {}
        finished = False
        for ls in range(learner_steps):
            # random selections with a share of deliberately valid / empty ones: invalid and empty selections both stay frequent
            view = np.stack([o[mask_slice] for o in observations]).astype(bool)
            bits = rng.random_sample((Nc, Nt)) < 0.3
            for c in range(Nc):
                u = rng.random_sample()
                if u < 0.5 and view[c].any():
                    bits[c] = view[c] & (rng.random_sample(Nt) < 0.7)
                    if not bits[c].any():
                        bits[c, np.flatnonzero(view[c])[0]] = True
                elif u < 0.65:
                    bits[c] = False
            if not multi:
                index = np.asarray([rng.choice(np.flatnonzero(b)) if b.any() else Nt for b in bits], dtype=np.int64)
                bits = np.eye(Nt + 1, Nt, dtype=bool)[index]
                action = index
            else:
                action = bits.astype(np.int64)
            current.update(bits=bits.copy(), ls=ls)
            del frames_of_fragment[:]
            first_frame = len(per_step.get('done', []))
            observations, rewards, dones, infos = env.step(action)
            frames = len(per_step['done']) - first_frame
            for f, frame_infos in enumerate(frames_of_fragment):      # the wrapper wrote its four metrics into every frame's infos
                push(per_step, 'metrics', np.asarray([[frame_infos[c][k] for k in METRICS] for c in range(Nc)], dtype=np.float64)
                     if (frame_skip == 1 or f < frames - 1) else last_frame_metrics(bits, per_step['view_after'][-1]))
            push(per_skip, 'selection_bits', bits)
            push(per_skip, 'selection', np.asarray(action))
            push(per_skip, 'frames', frames)
            push(per_skip, 'reward_cam', np.asarray(rewards, dtype=np.float64))
            push(per_skip, 'info_metrics', np.asarray([[infos[c][k] for k in METRICS] for c in range(Nc)], dtype=np.float64))
            push(per_skip, 'info_coverage_rate', np.float64(infos[0]['coverage_rate']))
            push(per_skip, 'action_mask', np.stack([env.action_mask(o) for o in observations]).astype(np.uint8))
            push(per_skip, 'done', bool(all(dones)))
            if all(dones):
                finished = True
                break
    finally:
        single_team.group_step = real_group_step
        gym.spaces.Box.sample = MG._ORIG_BOX_SAMPLE
    for k, v in per_step.items():
        out['step/' + k] = np.stack(v)
    for k, v in per_skip.items():
        out['skip/' + k] = np.stack(v)
    out.pop('step/state', None)
    sel, view = out['step/selection_bits'], out['step/view_before']
    empty = ~(sel & view).any(axis=-1)
    invalid = (sel & ~view).any(axis=-1)
    assert empty.mean() >= 0.10 and invalid.mean() >= 0.10, (name, empty.mean(), invalid.mean())
    assert (~empty).mean() >= 0.10, (name, (~empty).mean())      # (... and the executor's tracking branch as often)
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(f'{name}: {len(per_skip["done"])} fragments = {len(per_step["done"])} frames, finished={finished}, empty={empty.mean():.2f}, '
          f'invalid={invalid.mean():.2f}, {size / 1024:.0f} KiB')
    return out


def last_frame_metrics(bits, view_after):
    """The wrapper's per-frame metrics of a fragment's LAST frame, whose infos its MetricCollector overwrote with the fragment's
    means: the four numbers by their definition (wrappers.py:120-136) from the recorded selection and view."""
    sel = bits.sum(axis=-1)
    invalid = (bits & ~view_after).sum(axis=-1)
    return np.stack([sel, (bits & view_after).sum(axis=-1), invalid, invalid / np.maximum(1, sel)], axis=-1).astype(np.float64)


def main():
    selection_fixture('selection_4v8-9_multi_s31', 'MATE-4v8-9.yaml', 31, True, 1, 60, shaping=({'coverage_rate': 1.0}, 'mean'))
    selection_fixture('selection_4v2-9_single_s32', 'MATE-4v2-9.yaml', 32, False, 3, 40)
    # (max_episode_steps = 58: the episode ends on its 59th frame, the fourth frame of the twelfth fragment)
    selection_fixture('selection_2v4-0_multi_s33', 'MATE-2v4-0.yaml', 33, True, 5, 40, overrides={'max_episode_steps': 58})


if __name__ == '__main__':
    main()
