#!/usr/bin/env python3
"""Generator of tests/golden/message_*.npz: the reference's own send_messages / receive_messages / step under its channel wrappers -- mate.NoCommunication,
mate.RandomMessageDropout, mate.RestrictedCommunicationRange, stacked where the case says so -- with array contents sent by a scripted "learner", around the
reference's environment stepped under a random policy, through one episode end and the reset() behind it.  make_golden.py's machinery (the gym stand-in, the
recording RNG proxy, random_actions, drain_log, the snapshots) is imported, not edited; the dropout draws are attributed to their messages as
make_channel_golden.py does it, by a pass-through mate.MessageFilter directly outside the dropout wrapper.

Every step sends in up to two rounds, both teams in each: step % 4 == 0 one broadcast per agent, 1 addressed messages from a fixed pseudo-random address
matrix with a content per pair, 2 a broadcast round then an addressed round, 3 nothing.  (The range fixtures start 45 or 30 steps into their first episode, the
targets walked apart: under the random policy alone they never get 1400 apart in a few dozen steps.)  Behind every round receive_messages() is read, ahead of
every step() the *_communication_edges, behind it `info` and the *_total_communication_edges.

Keys beyond the scalars of a trace fixture (config_file ... target_step_size):
    channel/no_communication, channel/range_limit (-1: none), channel/dropout_rate
    ep<k>/static/*, ep<k>/reset/*     the state each of the two episodes starts from (make_golden.py's snapshots without knot tables and state vector)
    step/cam_act, step/tgt_act, step/goal_u, step/tgt_xy, step/done, step/episode      what moves the targets, where they are behind the step, the episode (0 / 1)
    msg/rounds [T], msg/broadcast [T, 2]
    per team tag (cam, tgt), [sender][recipient] but the inbox:
    msg/<tag>_xy [T, n, 2]              the locations the distances were taken from
    msg/<tag>_sent, _delivered [T, 2, n, n] int8;  msg/<tag>_u [T, 2, n, n] f64, NaN where no binomial was drawn
    msg/<tag>_payload [T, 2, n, n, M] f64 (a broadcast's content repeated over the recipients);  msg/<tag>_inbox [T, 2, n recipient, n sender, M]
    msg/<tag>_step_edges [T, n, n] ahead of step();  msg/<tag>_total_edges [T, n, n] behind it;  msg/<tag>_out, _in [T, n] of `info`
Arrays and names only are stored: data, no program text.  Every filtering fixture must show, per talking team, at least 3 delivered and 3 dropped messages
between different agents, and tests/message_ref.py must reproduce every recorded array.

    MATE_REFERENCE=<checkout of XuehaiPan/mate> python tests/golden/make_message_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (puts the shim and the reference on sys.path, imports gym and mate)
import message_ref as R  # noqa: E402

import mate  # noqa: E402
from mate.utils import Message, Team  # noqa: E402

WIDTH, ROUNDS = 4, 2


def snapshot(env):
    static = {k: v for k, v in MG.snapshot_static(env).items() if not k.startswith('lut_')}
    dynamic = {k: v for k, v in MG.snapshot_dynamic(env).items() if k != 'state'}
    return static, dynamic


def message_fixture(name, config, seed, steps, episode_steps, no_communication='none', range_limit=None, dropout_rate=None, warmup=0):
    """`warmup`: unrecorded steps ahead of the recording in which target t walks towards corner t % 4 of the terrain, so that the recorded steps of the first
    episode find the targets spread out (a range limit then has something to drop); the recording starts from the state they leave."""
    base = mate.make('MultiAgentTracking-v0', config=config, max_episode_steps=warmup + episode_steps)
    base.seed(seed)
    base.reset()
    corners = np.array([[900.0, 900.0], [-900.0, 900.0], [-900.0, -900.0], [900.0, -900.0]])
    for _ in range(warmup):
        heading = np.array([corners[t % 4] - target.location for t, target in enumerate(base.targets)])
        tgt_act = heading / np.maximum(np.linalg.norm(heading, axis=1, keepdims=True), 1e-9) * base.target_step_size
        assert not base.step((np.zeros((base.num_cameras, 2)), tgt_act))[2]
    log = []
    MG.install_proxies(base, log)
    Nc, Nt = base.num_cameras, base.num_targets
    sizes, tags, teams = (Nc, Nt), ('cam', 'tgt'), (Team.CAMERA, Team.TARGET)
    assert [t.value for t in teams] == [0, 1]

    ahead_of_dropout = []

    def note_dropout_input(unwrapped, message):
        ahead_of_dropout.append(message)
        return True

    env = base      # innermost first: dropout, its recorder, the range limit, NoCommunication
    if dropout_rate is not None:
        env = mate.MessageFilter(mate.RandomMessageDropout(env, dropout_rate), filter=note_dropout_input)
    if range_limit is not None:
        env = mate.RestrictedCommunicationRange(env, range_limit)
    if no_communication != 'none':
        env = mate.NoCommunication(env, team=no_communication)

    rng = np.random.RandomState(seed + 2000)
    address = [(rng.random_sample((n, n)) < 0.55).astype(np.uint8) for n in sizes]      # the fixed address matrices of the addressed rounds

    out = {'config_file': np.str_(config), 'seed': np.int64(seed), 'num_cameras': np.int64(Nc), 'num_targets': np.int64(Nt), 'num_obstacles': np.int64(base.num_obstacles),
           'transmittance': np.float64(base.obstacle_transmittance), 'max_episode_steps': np.int64(base.max_episode_steps), 'sparse_reward': np.bool_(base._sparse_reward),
           'freight_scale': np.float64(base.freight_scale), 'bounty_scale': np.float64(base.bounty_scale), 'reward_scale': np.float64(base.reward_scale),
           'max_target_team_episode_reward': np.float64(base.max_target_team_episode_reward), 'target_step_size': np.float64(base.target_step_size),
           'channel/no_communication': np.str_(no_communication), 'channel/range_limit': np.float64(-1.0 if range_limit is None else range_limit),
           'channel/dropout_rate': np.float64(0.0 if dropout_rate is None else dropout_rate), 'msg/width': np.int64(WIDTH)}
    for team, tag in enumerate(tags):
        out[f'msg/{tag}_address'] = address[team]

    def start_episode(k):
        static, dynamic = snapshot(base)
        for key, value in static.items():
            out[f'ep{k}/static/{key}'] = value
        for key, value in dynamic.items():
            out[f'ep{k}/reset/{key}'] = value
    start_episode(0)

    rows = {}

    def push(key, value):
        rows.setdefault(key, []).append(np.asarray(value))

    act_rng = np.random.RandomState(seed + 1000)
    episode, finished = 0, 0
    for step in range(steps):
        kind = step % 4
        plan = {0: ['broadcast'], 1: ['addressed'], 2: ['broadcast', 'addressed'], 3: []}[kind]
        now = {}
        for team, (tag, n) in enumerate(zip(tags, sizes)):
            entities = base.cameras if team == 0 else base.targets
            now[tag, 'xy'] = np.array([[x.location[0], x.location[1]] for x in entities], dtype=np.float64).reshape(n, 2)
            now[tag, 'sent'] = np.zeros((ROUNDS, n, n), dtype=np.int8)
            now[tag, 'delivered'] = np.zeros((ROUNDS, n, n), dtype=np.int8)
            now[tag, 'u'] = np.full((ROUNDS, n, n), np.nan)
            now[tag, 'payload'] = np.zeros((ROUNDS, n, n, WIDTH))
            now[tag, 'inbox'] = np.zeros((ROUNDS, n, n, WIDTH))
        for round_, how in enumerate(plan):
            for team, (tag, n) in enumerate(zip(tags, sizes)):
                messages = []
                if how == 'broadcast':
                    content = rng.randint(-800, 800, size=(n, WIDTH)) / 8.0      # (exact in f32)
                    now[tag, 'payload'][round_] = content[:, None, :]
                    now[tag, 'sent'][round_] = 1
                    messages = [Message(sender=s, recipient=None, content=content[s].copy(), team=teams[team], broadcasting=True) for s in range(n)]
                else:
                    content = rng.randint(-800, 800, size=(n, n, WIDTH)) / 8.0
                    now[tag, 'payload'][round_] = content
                    now[tag, 'sent'][round_] = address[team]
                    messages = [Message(sender=s, recipient=r, content=content[s, r].copy(), team=teams[team]) for s in range(n) for r in range(n) if address[team][s, r]]
                before = len(log)
                del ahead_of_dropout[:]
                if messages:
                    env.send_messages(messages)
                draws = [item for item in log[before:] if item[0] == 'binomial' and item[1] == 'env']
                assert len(draws) == len(log) - before == len(ahead_of_dropout)
                for m, (_, _, _, p, u, _) in zip(ahead_of_dropout, draws):
                    assert p == dropout_rate and np.isnan(now[tag, 'u'][round_, m.sender, m.recipient])
                    now[tag, 'u'][round_, m.sender, m.recipient] = u
                del log[before:]
            received = env.receive_messages()
            for team, (tag, n) in enumerate(zip(tags, sizes)):
                for r in range(n):
                    senders = [m.sender for m in received[team][r]]
                    assert senders == sorted(set(senders)) and all(m.recipient == r for m in received[team][r])      # at most one per pair, in sender order
                    for m in received[team][r]:
                        now[tag, 'delivered'][round_, m.sender, r] = 1
                        now[tag, 'inbox'][round_, r, m.sender] = m.content
        assert not any(len(q) for queues in base.message_queues for q in queues.values())
        for team, tag in enumerate(tags):
            edges = np.asarray(base.communication_edges[team]).astype(np.int32)
            assert np.array_equal(edges, now[tag, 'delivered'].sum(axis=0))
            push(f'msg/{tag}_step_edges', edges)
            for key in ('xy', 'sent', 'delivered', 'u', 'payload', 'inbox'):
                push(f'msg/{tag}_{key}', now[tag, key])
        push('msg/rounds', np.int64(len(plan)))
        push('msg/broadcast', np.array([how == 'broadcast' for how in plan] + [False] * (ROUNDS - len(plan))))

        cam_act, tgt_act = MG.random_actions(base, act_rng, step)
        log.clear()
        _, _, done, (cam_infos, tgt_infos) = base.step((cam_act, tgt_act))
        _, _, goal_u, _, _ = MG.drain_log(base, log)
        for team, (tag, infos) in enumerate(zip(tags, (cam_infos, tgt_infos))):
            push(f'msg/{tag}_out', np.array([info['out_communication_edges'] for info in infos], dtype=np.int32))
            push(f'msg/{tag}_in', np.array([info['in_communication_edges'] for info in infos], dtype=np.int32))
            assert [len(info['messages']) for info in infos] == list(now[tag, 'delivered'].sum(axis=(0, 1)))      # info's copies: everything of the step, per recipient
            totals = (base.camera_total_communication_edges, base.target_total_communication_edges)[team]
            push(f'msg/{tag}_total_edges', np.asarray(totals).astype(np.int32))
        push('step/cam_act', cam_act)
        push('step/tgt_act', tgt_act)
        push('step/goal_u', goal_u)
        push('step/tgt_xy', np.array([t.location for t in base.targets]).reshape(Nt, 2))
        push('step/done', done)
        push('step/episode', np.int64(episode))
        if done:
            finished += 1
            assert finished == 1, 'one episode end per fixture'
            base.reset()
            MG.install_proxies(base, log)
            log.clear()
            episode += 1
            start_episode(episode)
            for team in range(2):
                assert not np.asarray((base.camera_total_communication_edges, base.target_total_communication_edges)[team]).any()
    assert finished == 1 and episode == 1
    for key, value in rows.items():
        out[key] = np.stack(value)
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)

    # tests/message_ref.py reproduces the recording; the coverage the seeds were chosen for
    counts = []
    T = len(out['step/done'])
    for team, (tag, n) in enumerate(zip(tags, sizes)):
        if n == 0:
            counts.append((0, 0))
            continue
        disabled = no_communication in ('both', ('camera', 'target')[team])
        channel = {'disabled': disabled, 'range_limit': range_limit, 'dropout_rate': dropout_rate or 0.0}
        book = R.Counts(1, n)
        kept = dropped = 0
        off = ~np.eye(n, dtype=bool)
        for s in range(T):
            for k in range(int(out['msg/rounds'][s])):
                sent = out[f'msg/{tag}_sent'][s, k]
                keep = R.verdict(channel, out[f'msg/{tag}_u'][s, k][None], out[f'msg/{tag}_xy'][s][None], (1, n, n))
                inbox, sent_, delivered = R.route(out[f'msg/{tag}_payload'][s, k][None], sent[None], True, keep)
                assert np.array_equal(sent_[0], sent) and np.array_equal(delivered[0], out[f'msg/{tag}_delivered'][s, k]), (name, tag, s, k)
                assert np.array_equal(inbox[0], out[f'msg/{tag}_inbox'][s, k]), (name, tag, s, k)
                book.update(s, int(out['step/episode'][s]), delivered)
                kept += int((delivered[0] != 0)[off].sum())
                dropped += int(((sent != 0) & (delivered[0] == 0))[off].sum())
            if int(out['msg/rounds'][s]):
                assert np.array_equal(book.step_edges[0], out[f'msg/{tag}_step_edges'][s]), (name, tag, s)
                assert np.array_equal(book.total_edges[0] + book.step_edges[0], out[f'msg/{tag}_total_edges'][s]), (name, tag, s)
                assert np.array_equal(book.agent_edges[0, :, 0], out[f'msg/{tag}_out'][s]) and np.array_equal(book.agent_edges[0, :, 1], out[f'msg/{tag}_in'][s])
        counts.append((kept, dropped))
        if (dropout_rate is not None or range_limit is not None) and n > 1:
            assert kept >= 3 and dropped >= 3, (name, tag, kept, dropped)
        if range_limit is not None:      # no pair so close to the rim that a last-place difference of a replayed position could flip it
            assert np.abs(R.C.pair_distances(out[f'msg/{tag}_xy']) - range_limit).min() > 1e-6
    assert max(int(out[f'msg/{tag}_step_edges'].max(initial=0)) for tag in tags) <= 2      # two rounds of a pair within one step
    print(f'{name}: {T} steps, camera kept / dropped {counts[0]}, target kept / dropped {counts[1]}, {os.path.getsize(path) / 1024:.0f} KiB')


def main():
    MG.check_binomial_model()
    message_fixture('message_4v8-9_nocomm_target', 'MATE-4v8-9.yaml', 3, 26, 13, no_communication='target')
    message_fixture('message_4v8-9_drop30', 'MATE-4v8-9.yaml', 3, 26, 13, dropout_rate=0.3)
    message_fixture('message_4v8-9_drop70', 'MATE-4v8-9.yaml', 3, 26, 13, dropout_rate=0.7)
    message_fixture('message_4v8-9_range1400', 'MATE-4v8-9.yaml', 3, 26, 13, range_limit=1400.0, warmup=45)
    message_fixture('message_8v8-9_range1000', 'MATE-8v8-9.yaml', 5, 26, 13, range_limit=1000.0, warmup=30)
    message_fixture('message_8v8-9_range1000_drop30', 'MATE-8v8-9.yaml', 5, 26, 13, range_limit=1000.0, dropout_rate=0.3, warmup=30)


if __name__ == '__main__':
    main()
