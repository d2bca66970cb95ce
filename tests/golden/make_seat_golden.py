#!/usr/bin/env python3
"""Generator of tests/golden/seat_*.npz: the reference's own mate.SingleCamera / mate.SingleTarget (mate/wrappers/single_team.py, SingleTeamSingleAgent) around
the reference's environment -- a learner in ONE seat of its team, Greedy teammates in the other slots, Greedy opponents -- recorded step by step with
make_golden.py's machinery (the gym stand-in, the recording RNG proxies, AGENT_LOG, the recording Box.sample, tweak_few_cargoes).  make_golden.py is
imported, not edited.  The learner's actions are uniform draws of a seeded RandomState of this recorder.

Beyond the keys of greedy_*.npz (static/*, reset/*, step/* of the environment; step/agent_* the agents' draws in their TRUE-index slots -- NaN / -1 in the
seat's, which draws nothing --; agent/tgt_reset_sample_u; step/cam_act, step/tgt_act the joint actions the environment consumed, the learner's row included):
    seat/team          str      'camera' | 'target'
    seat/index         int64    the wrapper's index of this episode
    seat/shuffle       bool     shuffle_entities of the configuration
    reset/seat_obs     [D]      what the wrapper's reset() returned
    step/seat_obs      [T, D]   what the wrapper's step() returned
    step/seat_action   [T, 2]   the learner's action
    step/seat_reward   [T]      the wrapper's reward
Arrays and names only are stored: data, no program text.  A seed is accepted only if tests/seat_ref.py reproduces every recorded teammate action to 1e-9, the
camera fixtures show at least one 'state' message to the seat and at least one step where a teammate tracks a target it only knows from a message, and the
few-cargo target fixture at least one broadcast.

    MATE_REFERENCE=<checkout of XuehaiPan/mate> python tests/golden/make_seat_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (puts the shim and the reference on sys.path, imports gym and mate)
import seat_ref as S  # noqa: E402

import gym  # noqa: E402
import mate  # noqa: E402
from mate.agents import GreedyCameraAgent, GreedyTargetAgent  # noqa: E402
from mate.wrappers.single_team import group_reset  # noqa: E402


def drain_agents(agents_by_team, Nc, Nt):
    """make_golden.drain_agent_log with the arrays sized by the TEAMS, not by the agents present: the seat's slots stay NaN / -1."""
    spaces_of = {id(a.action_space): (team, a.index) for team, agents in agents_by_team.items() for a in agents}
    out = {'cam_binom_u': np.full(Nc, np.nan), 'cam_sample_u': np.full((Nc, 2), np.nan), 'cam_delay': np.full((Nc, Nc), -1, dtype=np.int64),
           'tgt_choice_u': np.full(Nt, np.nan), 'tgt_binom_u': np.full(Nt, np.nan), 'tgt_sample_u': np.full((Nt, 2), np.nan)}
    for item in MG.AGENT_LOG:
        if item[0] == 'sample':
            if item[1] in spaces_of:
                team, idx = spaces_of[item[1]]
                out[team + '_sample_u'][idx] = item[2]
            continue
        team, idx = item[1]
        if item[0] == 'binom':
            out[team + '_binom_u'][idx] = item[3]
        elif item[0] == 'choice':
            out['tgt_choice_u'][idx] = (item[3] + 0.5) / item[2]
        elif item[0] == 'randint':
            assert team == 'cam' and item[5] is not None
            out['cam_delay'][idx, item[5]] = item[4]
    MG.AGENT_LOG.clear()
    return out


def seat_fixture(name, wrapper, config, seed, steps, overrides=None, tweak=None):
    camera = wrapper == 'SingleCamera'
    base = mate.make('MultiAgentTracking-v0', config=config, **(overrides or {}))
    if camera:
        env = mate.SingleCamera(base, other_camera_agent=GreedyCameraAgent(seed=seed + 1), target_agent=GreedyTargetAgent(seed=seed + 2))
    else:
        env = mate.SingleTarget(base, other_target_agent=GreedyTargetAgent(seed=seed + 2), camera_agent=GreedyCameraAgent(seed=seed + 1))
    env.seed(seed)
    everyone = list(env.teammate_agents_ordered) + list(env.opponent_agents_ordered)
    gym.spaces.Box.sample = MG._recording_box_sample
    try:
        for agent in everyone:
            agent._np_random = MG.AgentRNG(agent.np_random, MG.AGENT_LOG, None)
        MG.AGENT_LOG.clear()
        seat_obs = env.reset()
        if tweak is not None:      # state injection on the reference objects, then the wrapper's own resets of its agents again on the new observations
            tweak(base)
            joint = base.joint_observation()
            env.joint_observation, env.opponent_joint_observation = (joint[0], joint[1]) if camera else (joint[1], joint[0])
            MG.AGENT_LOG.clear()
            group_reset(env.opponent_agents, env.opponent_joint_observation)
            group_reset(env.teammate_agents, [row for i, row in enumerate(env.joint_observation) if i != env.index])
            seat_obs = env.joint_observation[env.index]
        z = int(env.index)
        Nc, Nt = base.num_cameras, base.num_targets
        cams = [a for a in everyone if isinstance(a, GreedyCameraAgent)]
        tgts = [a for a in everyone if isinstance(a, GreedyTargetAgent)]
        assert sorted(a.index for a in cams) == [c for c in range(Nc) if not (camera and c == z)]
        assert sorted(a.index for a in tgts) == [t for t in range(Nt) if camera or t != z]
        for a in cams:
            a._np_random._who = ('cam', a.index)
        for a in tgts:
            a._np_random._who = ('tgt', a.index)
        by_team = {'cam': cams, 'tgt': tgts}
        reset_draws = drain_agents(by_team, Nc, Nt)
        log = []
        MG.install_proxies(base, log)
        out = {'config_file': np.str_(config), 'seed': np.int64(seed), 'policy': np.str_(wrapper), 'num_cameras': np.int64(Nc), 'num_targets': np.int64(Nt),
               'num_obstacles': np.int64(base.num_obstacles), 'transmittance': np.float64(base.obstacle_transmittance),
               'max_episode_steps': np.int64(base.max_episode_steps), 'sparse_reward': np.bool_(base._sparse_reward),
               'freight_scale': np.float64(base.freight_scale), 'bounty_scale': np.float64(base.bounty_scale), 'reward_scale': np.float64(base.reward_scale),
               'max_target_team_episode_reward': np.float64(base.max_target_team_episode_reward), 'target_step_size': np.float64(base.target_step_size),
               'seat/team': np.str_('camera' if camera else 'target'), 'seat/index': np.int64(z), 'seat/shuffle': np.bool_(base.shuffle_entities),
               'agent/tgt_reset_sample_u': reset_draws['tgt_sample_u'], 'reset/seat_obs': np.asarray(seat_obs, dtype=np.float64)}
        if overrides and set(overrides) - {'max_episode_steps'}:
            out['overrides'] = np.str_(json.dumps(overrides, sort_keys=True))
        for k, v in MG.snapshot_static(base).items():
            out['static/' + k] = v
        for k, v in MG.snapshot_dynamic(base).items():
            out['reset/' + k] = v
        rng = np.random.RandomState(seed + 1000)
        high = np.array([base.camera_rotation_step, base.camera_zooming_step]) if camera else np.array([1.0, 1.0])
        per_step = {}

        def push(key, value):
            per_step.setdefault(key, []).append(np.asarray(value))

        consumed = {}
        original_step = base.step

        def recording_step(action):
            consumed['cam'], consumed['tgt'] = (np.asarray(a, dtype=np.float64).reshape(-1, 2) for a in action)
            return original_step(action)
        base.step = recording_step
        for step in range(steps):
            scale = high if camera else high * base.targets[z].step_size
            action = rng.uniform(-1.0, 1.0, size=2) * scale
            log.clear()
            seat_obs, reward, done, _ = env.step(action)
            for k, v in drain_agents(by_team, Nc, Nt).items():
                push('agent_' + k, v)
            tape_ct, _, goal_u, goal_k, goal_j = MG.drain_log(base, log)
            for key, value in (('cam_act', consumed['cam']), ('tgt_act', consumed['tgt']), ('tape_ct', tape_ct), ('goal_u', goal_u), ('goal_k', goal_k),
                               ('goal_j', goal_j), ('seat_obs', np.asarray(seat_obs, dtype=np.float64)), ('seat_action', action), ('seat_reward', np.float64(reward)),
                               ('done', bool(done))):
                push(key, value)
            for k, v in MG.snapshot_dynamic(base).items():
                if k != 'state':
                    push(k, v)
            if done:
                break
    finally:
        gym.spaces.Box.sample = MG._ORIG_BOX_SAMPLE
    for k, v in per_step.items():
        out['step/' + k] = np.stack(v)
    assert np.array_equal(out['step/' + ('cam_act' if camera else 'tgt_act')][:, z], out['step/seat_action'])
    return out, z


# name -> (wrapper, config, steps, overrides, tweak, candidate seeds)
CASES = {
    'seat_camera_4v8-9': ('SingleCamera', 'MATE-4v8-9.yaml', 96, {'shuffle_entities': False}, None, range(70, 90)),
    'seat_camera_8v8-9_shuffle': ('SingleCamera', 'MATE-8v8-9.yaml', 80, {'shuffle_entities': True}, None, range(70, 110)),
    'seat_target_4v8-9': ('SingleTarget', 'MATE-4v8-9.yaml', 96, {'shuffle_entities': False}, None, range(70, 90)),
    'seat_target_4v8-9_fewcargo': ('SingleTarget', 'MATE-4v8-9.yaml', 160, {'shuffle_entities': False}, MG.tweak_few_cargoes, range(70, 110)),
}


def accepted(name, fx, z):
    wrapper, _, _, overrides, tweak, _ = CASES[name]
    n = int(fx['num_cameras'] if wrapper == 'SingleCamera' else fx['num_targets'])
    if overrides and overrides.get('shuffle_entities') and z in (0, n - 1):
        return False, 'seat %d is an end slot' % z
    if not (overrides and overrides.get('shuffle_entities')) and z != n - 1:
        return False, 'seat %d is not n - 1' % z
    worst, total = S.replay(fx)
    if worst > 1e-9:
        return False, 'seat_ref misses the recorded actions by %g' % worst
    if wrapper == 'SingleCamera' and (total['state_to_seat'] < 1 or total['told'] < 1):
        return False, 'coverage %r' % total
    if tweak is not None and total['broadcasts'] < 1:
        return False, 'no broadcast'
    return True, 'worst %.3g, %r' % (worst, total)


def main():
    for name, (wrapper, config, steps, overrides, tweak, seeds) in CASES.items():
        for seed in seeds:
            fx, z = seat_fixture(name, wrapper, config, seed, steps, overrides, tweak)
            ok, why = accepted(name, fx, z)
            print(f'{name}: seed {seed}, seat {z}: {"accepted" if ok else "rejected"} ({why})')
            if ok:
                path = os.path.join(HERE, name + '.npz')
                np.savez_compressed(path, **fx)
                print(f'  {len(fx["step/done"])} steps, {os.path.getsize(path) / 1024:.0f} KiB')
                assert os.path.getsize(path) < 1 << 20
                break
        else:
            raise SystemExit(f'{name}: no seed accepted')


if __name__ == '__main__':
    main()
