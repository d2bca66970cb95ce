#!/usr/bin/env python3
"""Generator of tests/golden/naive_*.npz and random_*.npz: the reference's NaiveCameraAgent / NaiveTargetAgent (mate/agents/naive.py) and
RandomCameraAgent / RandomTargetAgent (mate/agents/random.py) playing both teams, recorded step by step with make_golden.py's machinery -- the gym
stand-in, the recording Box.sample and make_trace(..., policy='greedy', record_agents=True), whose `GreedyCameraAgent` / `GreedyTargetAgent` names are
pointed at the other pair for the duration of the trace.  make_golden.py is imported, not edited: its AgentRNG is subclassed HERE for the two draws
the Greedy agents never make (np_random.uniform of the Naive cameras; np_random.choice inside an agent's reset, where the proxy has no owner yet),
which go to a log of this module, keyed by the proxy object.

mixture_4v8-9.npz: MixtureTargetAgent([Greedy, Naive, Random], [1, 2, 1]) through 8 episodes of 12 steps of ONE environment object, every episode a
whole fixture under ep<k>/ (reset state, tapes, actions, the acting candidate's draws) with the candidate drawn and the uniform its choice(p=)
consumed (mixture_fixture below).

Beyond the keys of greedy_*.npz:
    step/agent_cam_uniform_u [T, Nc]       the Naive cameras' uniform (NaN for the Random pair)
    agent/tgt_reset_choice   [Nt, 2]       the Naive targets' reset: goal, inc
Arrays and names only are stored: data, no program text.  A fixture is accepted only if the restatement of tests/scripted_ref.py reproduces every
recorded action to 1e-9 and no branch condition of any recorded target-step lies within 1e-9 (relative) of equality; naive_4v8-9 must show both
arrival forms (its state injection zeroes remaining_cargoes[1] and [2], as tweak_few_cargoes injects), a skip over more than one warehouse and both
noise probabilities.

    MATE_REFERENCE=<checkout of XuehaiPan/mate> python tests/golden/make_scripted_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (puts the shim and the reference on sys.path, imports gym and mate)
import scripted_ref as R  # noqa: E402

from mate.agents.naive import NaiveCameraAgent, NaiveTargetAgent  # noqa: E402
from mate.agents.random import RandomCameraAgent, RandomTargetAgent  # noqa: E402

SIDE_LOG = []      # (proxy, 'uniform' | 'choice', value)


class ScriptedRNG(MG.AgentRNG):
    def uniform(self, low=0.0, high=1.0, size=None):
        assert size is None
        u = float(self._real.random_sample())
        SIDE_LOG.append((self, 'uniform', u))
        return low + (high - low) * u

    side_choice = True      # np_random.choice goes to this module's log (False: to make_golden's, as the Greedy targets' per-step choice must)

    def choice(self, a, size=None, replace=True, p=None):
        if not self.side_choice:
            return super().choice(a, size=size, replace=replace, p=p)
        assert size is None and p is None
        a = list(range(a)) if isinstance(a, (int, np.integer)) else list(a)
        j = int(self._real.randint(0, len(a)))
        SIDE_LOG.append((self, 'choice', a[j]))
        return a[j]


def empty_two_warehouses(env):
    env.remaining_cargoes[1].fill(0)
    env.remaining_cargoes[2].fill(0)
    for w in range(4):
        env.awaiting_cargo_counts[w] = env.remaining_cargoes[:, w].sum() + env.target_goal_bits[:, w].sum()
    env._state = None


def scripted_fixture(name, config, seed, steps, pair, tweak=None):
    camera_class, target_class = {'naive': (NaiveCameraAgent, NaiveTargetAgent), 'random': (RandomCameraAgent, RandomTargetAgent)}[pair]
    saved = MG.GreedyCameraAgent, MG.GreedyTargetAgent, MG.AgentRNG, MG.drain_agent_log
    drained = []

    def drain(cam_agents, tgt_agents):
        out = saved[3](cam_agents, tgt_agents)
        owner = {id(a._np_random): ('cam', a.index) for a in cam_agents}
        owner.update({id(a._np_random): ('tgt', a.index) for a in tgt_agents})
        uniform = np.full(len(cam_agents), np.nan)
        choices = {}
        for proxy, kind, value in SIDE_LOG:
            team, index = owner[id(proxy)]
            if kind == 'uniform':
                assert team == 'cam'
                uniform[index] = value
            else:
                assert team == 'tgt'
                choices.setdefault(index, []).append(value)
        SIDE_LOG.clear()
        drained.append(choices)
        out['cam_uniform_u'] = uniform
        return out

    MG.GreedyCameraAgent, MG.GreedyTargetAgent, MG.AgentRNG, MG.drain_agent_log = camera_class, target_class, ScriptedRNG, drain
    SIDE_LOG.clear()
    try:
        MG.make_trace(name, config, seed, 'greedy', steps, record_agents=True, tweak=tweak)
    finally:
        MG.GreedyCameraAgent, MG.GreedyTargetAgent, MG.AgentRNG, MG.drain_agent_log = saved
    path = os.path.join(HERE, name + '.npz')
    out = dict(np.load(path))
    Nt = int(out['num_targets'])
    out['policy'] = np.str_(pair)
    if pair == 'naive':
        assert sorted(drained[0]) == list(range(Nt)) and all(len(v) == 2 for v in drained[0].values()) and not any(drained[1:])
        out['agent/tgt_reset_choice'] = np.array([drained[0][t] for t in range(Nt)], dtype=np.int64)
    else:
        assert not any(drained)
    for key in ('reset/cam_obs', 'reset/tgt_obs', 'reset/state', 'step/target_warehouse_distances', 'step/target_obstacle_view_mask',
                'step/target_target_view_mask', 'step/camera_camera_view_mask', 'step/agent_cam_delay', 'step/agent_tgt_choice_u', 'step/agent_cam_binom_u'):
        out.pop(key, None)
    stats = check_fixture(out)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(f'{name}: {len(out["step/done"])} steps, {stats}, {size / 1024:.0f} KiB')
    return out, stats


def check_fixture(fx):
    """The restatement over the recording (tests/test_scripted_host.py runs the same function): worst difference, branch census, smallest margin."""
    got = R.replay_fixture(fx)
    assert got['worst'] < 1e-9, got['worst']
    assert got['margin'] > 1e-9, got['margin']
    return {k: v for k, v in got.items() if k not in ('cam', 'tgt')}


class _Population:
    """What make_trace takes for `GreedyTargetAgent`: called with a seed it returns itself, spawn() returns the SAME mixture agents in every episode."""

    def __init__(self, agents):
        self.agents = agents

    def __call__(self, seed=None):
        return self

    def spawn(self, count):
        assert count == len(self.agents)
        return self.agents


def mixture_fixture(name, config, seed, episodes=8, steps=12):
    """MixtureTargetAgent([Greedy, Naive, Random], [1, 2, 1]) as the target team of ONE environment object through `episodes` episodes of `steps` steps
    (max_episode_steps = steps) against the Greedy cameras, every episode recorded by make_trace from the reset() in front of it: ep<k>/... holds a
    whole fixture in the format of naive_*.npz -- the reset state, the occlusion tables, the environment's tapes, both teams' actions, the draws of
    the candidate that played, through the recording proxies -- plus ep<k>/choice (the candidate, an index into `candidates`) and ep<k>/uniform (what
    np_random_mixture.choice(p=) consumed, read from a COPY of the generator's state just before the agents' reset: the reference's own choice() runs
    untouched).  An episode is accepted only if the restatement reproduces the recorded actions of a Naive or Random episode to 1e-9 with no branch
    condition within 1e-9 of equality (a Greedy episode's rows are the Greedy agents' own: tests/test_gpu_policies.py holds those)."""
    from mate.agents.mixture import MixtureTargetAgent
    mate = MG.mate
    env = mate.make('MultiAgentTracking-v0', config=config, max_episode_steps=steps)
    env.seed(seed)
    weights = [1.0, 2.0, 1.0]
    classes = (MG.GreedyTargetAgent, NaiveTargetAgent, RandomTargetAgent)
    names = ['greedy', 'naive', 'random']
    agents = MixtureTargetAgent(candidates=[c() for c in classes], weights=weights, seed=seed + 2).spawn(env.num_targets)
    for index, agent in enumerate(agents):
        for candidate in agent.candidates:
            proxy = ScriptedRNG(candidate.np_random, MG.AGENT_LOG, ('tgt', index))
            proxy.side_choice = isinstance(candidate, NaiveTargetAgent)      # (the Greedy targets' per-step choice is make_golden's to record)
            candidate._np_random = proxy
    saved = MG.GreedyTargetAgent, MG.drain_agent_log
    drained = []

    def drain(cam_agents, tgt_agents):
        out = saved[1](cam_agents, [a.current_agent for a in tgt_agents])      # (the action spaces and indices of the agents that act)
        choices = {}
        for proxy, kind, value in SIDE_LOG:
            assert kind == 'choice'
            choices.setdefault(proxy._who[1], []).append(value)
        SIDE_LOG.clear()
        drained.append(choices)
        return out

    out = dict(config_file=np.str_(config), seed=np.int64(seed), policy=np.str_('mixture_target'), weights=np.asarray(weights),
               candidates=np.asarray(names), max_episode_steps=np.int64(steps), episodes=np.int64(episodes))
    played = []
    MG.GreedyTargetAgent, MG.drain_agent_log = _Population(agents), drain
    try:
        for episode in range(episodes):
            first_obs = env.reset()
            us = []
            for agent in agents:
                probe = np.random.RandomState()
                probe.set_state(agent.np_random_mixture.get_state())
                us.append(float(probe.random_sample()))
            del drained[:]
            SIDE_LOG.clear()
            tag = f'{name}_ep{episode}'
            MG.make_trace(tag, config, seed, 'greedy', steps, record_agents=True, env=env, first_obs=first_obs)
            path = os.path.join(HERE, tag + '.npz')
            fx = dict(np.load(path))
            os.remove(path)
            choice = [classes.index(type(agent.current_agent)) for agent in agents]
            assert len(set(choice)) == 1, 'spawn() seeds a team alike: one candidate per episode'
            assert np.array_equal(R.mixture_choice(weights, us), choice)
            assert len(fx['step/done']) == steps
            fx['policy'] = np.str_(names[choice[0]])
            if names[choice[0]] == 'naive':
                assert sorted(drained[0]) == list(range(env.num_targets)) and all(len(v) == 2 for v in drained[0].values()) and not any(drained[1:])
                fx['agent/tgt_reset_choice'] = np.array([drained[0][t] for t in range(env.num_targets)], dtype=np.int64)
                fx['step/agent_cam_uniform_u'] = np.full(fx['step/agent_cam_binom_u'].shape, np.nan)
            else:
                assert not any(drained)
            for key in ('reset/cam_obs', 'reset/tgt_obs', 'reset/state', 'step/target_warehouse_distances', 'step/target_obstacle_view_mask',
                        'step/target_target_view_mask', 'step/camera_camera_view_mask', 'static/lut_outer_phis', 'static/lut_outer_rhos', 'static/lut_outer_count'):
                fx.pop(key, None)
            if names[choice[0]] != 'greedy':
                got = R.replay_fixture(fx, teams=(1,))
                assert got['worst'] < 1e-9 and got['margin'] > 1e-9, (episode, got['worst'], got['margin'])
            fx['choice'], fx['uniform'] = np.asarray(choice, dtype=np.int64), np.asarray(us)
            out.update({f'ep{episode}/{k}': v for k, v in fx.items()})
            played.append(choice[0])
    finally:
        MG.GreedyTargetAgent, MG.drain_agent_log = saved
    assert len(set(played)) == 3, played      # every candidate plays some episode
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(f'{name}: choices {played}, {size / 1024:.0f} KiB')
    return out


def main():
    # seed 5 and its successors show both arrival forms and both probabilities under the recording proxies, but no skip over two warehouses before seed 48:
    # the first seed that shows every branch is taken
    for seed in (48,) + tuple(range(5, 100)):
        try:
            _, stats = scripted_fixture('naive_4v8-9', 'MATE-4v8-9.yaml', seed, 500, 'naive', tweak=empty_two_warehouses)
            assert stats['once'] > 0 and stats['skip'] > 0 and stats['far'] > 0 and stats['p05'] > 0 and stats['p75'] > 0, stats
            break
        except AssertionError as err:
            print('seed', seed, 'rejected:', err)
    else:
        raise SystemExit('no seed gave every branch')
    scripted_fixture('naive_2v4-0', 'MATE-2v4-0.yaml', 6, 200, 'naive')
    scripted_fixture('naive_8v8-9', 'MATE-8v8-9.yaml', 7, 200, 'naive')
    scripted_fixture('random_4v8-9', 'MATE-4v8-9.yaml', 8, 70, 'random')
    scripted_fixture('random_2v4-0', 'MATE-2v4-0.yaml', 9, 70, 'random')
    for seed in range(10, 40):       # the first seed whose eight episodes show all three candidates
        try:
            mixture_fixture('mixture_4v8-9', 'MATE-4v8-9.yaml', seed)
            break
        except AssertionError as err:
            print('mixture seed', seed, 'rejected:', err)
    else:
        raise SystemExit('no seed gave every candidate')


if __name__ == '__main__':
    main()
