#!/usr/bin/env python3
"""Generator of tests/golden/heuristic_*.npz: the reference's HeuristicTargetAgent (mate/agents/heuristic.py:290-337) playing the
targets against GreedyCameraAgent, recorded step by step with make_golden.py's machinery -- the gym stand-in, the recording RNG
proxies and make_trace(..., policy='greedy', record_agents=True), whose `GreedyTargetAgent` name is pointed at the heuristic class for
the duration of the trace.

Beyond the keys of greedy_*.npz every step carries
    step/tgt_act_greedy   what GreedyTargetAgent.act returned inside HeuristicTargetAgent.act (the class attribute is wrapped HERE, in this
                          process; the reference's files are not touched)
    step/tgt_act          the final action (make_trace's own key)
Arrays and names only are stored: data, no program text.  Seeds are accepted only if the restatement of tests/heuristic_ref.py
reproduces every recorded final action to 1e-9, every branch of the drift is exercised and no branch condition of any recorded
target-step lies within 1e-9 (relative) of equality.

    MATE_REFERENCE=<checkout of XuehaiPan/mate> python tests/golden/make_heuristic_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (puts the shim and the reference on sys.path, imports gym and mate)
from heuristic_ref import fixture_inputs, heuristic_drift  # noqa: E402

from mate.agents.heuristic import HeuristicTargetAgent  # noqa: E402


def heuristic_fixture(name, config, seed, steps):
    greedy_class = MG.GreedyTargetAgent
    real_act = greedy_class.act
    greedy_actions = []

    def recording_act(self, observation, info=None, deterministic=None):
        action = real_act(self, observation, info, deterministic=deterministic)
        greedy_actions.append((self.index, np.array(action, dtype=np.float64)))
        return action

    greedy_class.act = recording_act
    MG.GreedyTargetAgent = HeuristicTargetAgent
    try:
        MG.make_trace(name, config, seed, 'greedy', steps, record_agents=True)
    finally:
        MG.GreedyTargetAgent = greedy_class
        greedy_class.act = real_act
    path = os.path.join(HERE, name + '.npz')
    out = dict(np.load(path))
    T, Nt = len(out['step/done']), int(out['num_targets'])
    assert len(greedy_actions) == T * Nt and [i for i, _ in greedy_actions] == list(range(Nt)) * T
    out['step/tgt_act_greedy'] = np.stack([a for _, a in greedy_actions]).reshape(T, Nt, 2)
    out['policy'] = np.str_('heuristic_target')
    # what no test of this fixture reads (the keys make_trace itself drops for the agents' fixtures aside): keep the file small
    for key in ('reset/cam_obs', 'reset/tgt_obs', 'reset/state', 'step/target_warehouse_distances', 'step/target_obstacle_view_mask',
                'step/target_target_view_mask', 'step/camera_camera_view_mask'):
        out.pop(key, None)
    final, info = heuristic_drift(**fixture_inputs(out))
    worst = float(np.abs(final - out['step/tgt_act']).max())
    sensing = fixture_inputs(out)['sensed'].any(axis=-1)
    drifted, rejected = info['drifted'], info['rejected']
    margin = float(info['margin'].min())
    print(f'{name}: {T} steps, |restatement - recorded| = {worst:.2e}, sensing {sensing.mean():.2f}, drifted {drifted.mean():.3f} '
          f'({drifted.sum() / max(1, sensing.sum()):.2f} of sensing), dot-rejected {rejected.mean():.3f}, clipped {int(info["clipped"].sum())}, '
          f'two or more candidates {int((info["candidates"] >= 2).sum())}, smallest branch margin {margin:.2e}')
    assert worst < 1e-9, worst
    assert drifted.mean() >= 0.20 and rejected.mean() >= 0.02 and info['clipped'].any(), name
    assert margin > 1e-9, margin
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(f'    {size / 1024:.0f} KiB')
    return out


def main():
    heuristic_fixture('heuristic_4v8-9_s51', 'MATE-4v8-9.yaml', 51, 160)
    out = heuristic_fixture('heuristic_8v8-9_s52', 'MATE-8v8-9.yaml', 52, 120)
    final, info = heuristic_drift(**fixture_inputs(out))
    assert (info['candidates'] >= 2).any(), 'the 8v8-9 fixture must exercise the minimum rule'
    heuristic_fixture('heuristic_4v2-9_s53', 'MATE-4v2-9.yaml', 53, 160)


if __name__ == '__main__':
    main()
