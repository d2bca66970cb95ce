#!/usr/bin/env python3
"""Generator of tests/golden/fragment_*.npz: the tail of the reference's example trainer chains

    MultiCamera | MultiTarget (greedy opponent) -> RelativeCoordinates -> RescaledObservation -> RepeatedRewardIndividualDone
        -> [AuxiliaryCameraRewards] -> FrameSkip(K)

driven on the CPU, fragment by fragment.  Imports the upstream reference read-only (its checkout is named by the MATE_REFERENCE
environment variable) under the `gymshim` package next to this file.  FrameSkip itself lives in `examples.utils`, which needs ray: the
fragment loop below is a stand-in written here (hold the action for up to K frames, stop when every agent is done, sum the reward
rows, reduce the infos by sum / mean / last as FrameSkip.INFO_KEYS names them).  Arrays and names only are stored: data, no program text.

Per frame (the base environment's step, wrapped): the learner team's PLAIN observation rows, the eight values of the engine's scalar
record as f64 (camera team reward, target team reward, done, coverage_rate, real_coverage_rate, mean_transport_rate,
num_delivered_cargoes, normalised target team reward), the camera -> target view bits packed as the engine packs them
(bit c * Nt + t, 32 per word).  Per fragment: the chain's observation, reward and done rows, the reduced infos, the frames that ran.
An episode is cut short (max_episode_steps) so that it ends on an inner frame of a fragment; the next fragment starts a new episode.

    MATE_REFERENCE=<checkout of XuehaiPan/mate> python tests/golden/make_fragment_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the shim and the reference on sys.path, imports gym and mate)

mate = MG.mate
if not hasattr(np, 'bool8'):
    np.bool8 = np.bool_

INFO_SUM, INFO_MEAN, INFO_LAST = ('raw_reward', 'normalized_raw_reward'), ('coverage_rate', 'real_coverage_rate'), ('mean_transport_rate', 'num_delivered_cargoes')


def pack_view(view):
    bits = np.asarray(view, dtype=bool).reshape(-1)
    words = np.zeros((bits.size + 31) // 32, dtype=np.uint32)
    for i in np.flatnonzero(bits):
        words[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return words


def fragment_fixture(name, config, seed, learner, frame_skip, episodes, max_episode_steps, shaping=None):
    base = mate.make('MultiAgentTracking-v0', config=config, reward_type='dense', max_episode_steps=max_episode_steps)
    if learner == 'camera':
        env = mate.MultiCamera(base, target_agent=MG.GreedyTargetAgent(seed=0))
    else:
        env = mate.MultiTarget(base, camera_agent=MG.GreedyCameraAgent(seed=0))
    env = mate.RepeatedRewardIndividualDone(mate.RescaledObservation(mate.RelativeCoordinates(env)))
    if shaping is not None:
        env = mate.AuxiliaryCameraRewards(env, coefficients=shaping[0], reduction=shaping[1])
    env.seed(seed)
    frames = []
    real_step = base.step

    def recording_step(action):
        observation, reward, done, info = real_step(action)
        rows = np.asarray(observation[0 if learner == 'camera' else 1], dtype=np.float64)
        common = info[1][0]
        scalars = np.asarray([reward[0], reward[1], float(done), common['coverage_rate'], common['real_coverage_rate'], common['mean_transport_rate'],
                              common['num_delivered_cargoes'], common['normalized_raw_reward']], dtype=np.float64)
        frames.append((rows, scalars, pack_view(base.camera_target_view_mask)))
        return observation, reward, done, info

    base.step = recording_step
    rng = np.random.RandomState(seed + 1000)
    agents = base.num_cameras if learner == 'camera' else base.num_targets
    high = np.asarray((base.camera_action_space if learner == 'camera' else base.target_action_space).high, dtype=np.float64)
    out = {key: [] for key in ('frame/rows', 'frame/scalars', 'frame/view_words', 'skip/first_frame', 'skip/frames', 'skip/obs', 'skip/rewards',
                               'skip/dones', 'skip/info', 'skip/action')}
    for episode in range(episodes):
        env.reset()
        finished = False
        while not finished:
            action = rng.uniform(-1.0, 1.0, size=(agents, 2)) * high
            first, rewards, infos_seen = len(frames), [], []
            for f in range(frame_skip):                    # the stand-in for FrameSkip.step
                observations, reward, dones, infos = env.step(action)
                rewards.append(reward)
                infos_seen.append(infos[0])
                if all(dones):
                    break
            finished = all(dones)
            reduced = [np.sum([i[k] for i in infos_seen]) for k in INFO_SUM] + [np.mean([i[k] for i in infos_seen]) for k in INFO_MEAN] + \
                      [infos_seen[-1][k] for k in INFO_LAST]
            out['skip/first_frame'].append(first)
            out['skip/frames'].append(len(frames) - first)
            out['skip/obs'].append(np.asarray(observations, dtype=np.float64))
            out['skip/rewards'].append(np.sum(rewards, axis=0))
            out['skip/dones'].append(np.asarray(dones, dtype=bool))
            out['skip/info'].append(np.asarray(reduced, dtype=np.float64))
            out['skip/action'].append(action)
    out['frame/rows'], out['frame/scalars'], out['frame/view_words'] = ([f[k] for f in frames] for k in range(3))
    fx = {key: np.asarray(value) for key, value in out.items()}
    counts = fx['skip/frames']
    assert (counts < frame_skip).any() and (counts == frame_skip).any(), counts
    fx.update({
        'config_file': np.str_(config), 'seed': np.int64(seed), 'learner_team': np.str_(learner), 'frame_skip': np.int64(frame_skip),
        'num_cameras': np.int64(base.num_cameras), 'num_targets': np.int64(base.num_targets), 'num_obstacles': np.int64(base.num_obstacles),
        'max_episode_steps': np.int64(max_episode_steps), 'info_names': np.asarray(INFO_SUM + INFO_MEAN + INFO_LAST),
    })
    if shaping is not None:
        fx['aux_keys'] = np.asarray(list(shaping[0].keys()))
        fx['aux_coefficients'] = np.asarray(list(shaping[0].values()), dtype=np.float64)
        fx['aux_reduction'] = np.str_(shaping[1])
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **fx)
    print(name, 'frames per fragment', counts.tolist(), os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    fragment_fixture('fragment_4v8-9_camera_s41', 'MATE-4v8-9.yaml', 41, 'camera', 5, episodes=2, max_episode_steps=12,
                     shaping=({'coverage_rate': 1.0, 'num_tracked': 0.25}, 'mean'))
    fragment_fixture('fragment_2v4-0_target_s42', 'MATE-2v4-0.yaml', 42, 'target', 10, episodes=2, max_episode_steps=24)
