#!/usr/bin/env python3
"""Generator of tests/golden/channel_*.npz: the reference's own channel wrappers -- mate.NoCommunication, mate.RandomMessageDropout,
mate.RestrictedCommunicationRange, stacked where the case says so -- around the reference's environment, GreedyCameraAgent versus GreedyTargetAgent
under group_step, recorded step by step with make_golden.py's machinery (the gym stand-in, the recording RNG proxies, AGENT_LOG, make_trace(...,
policy='greedy', record_agents=True), tweak_few_cargoes).  make_golden.py is imported, not edited.

make_trace steps the BASE environment object; the wrappers are put in the agents' way by an instance attribute `send_messages` on that object, which
hands every call to the outermost wrapper and lets the innermost one through to the class's own method.  Two pass-through mate.MessageFilter objects
record what passes: one outside everything (`sent`), one directly outside the dropout wrapper (the messages its binomial draws belong to, in order).
`delivered` is read from the base environment's camera_ / target_communication_edges ahead of every step, and must equal what reached the base method.

Beyond the keys of greedy_*.npz:
    channel/no_communication  str       'both' | 'camera' | 'target' | 'none'
    channel/range_limit       f64       -1: none
    channel/dropout_rate      f64
    step/chan_cam_sent, step/chan_cam_delivered  [T, Nc, Nc] int8, [sender][recipient]
    step/chan_tgt_sent, step/chan_tgt_delivered  [T, Nt, Nt] int8
    step/chan_cam_u, step/chan_tgt_u             [T, n, n] f64: the uniform of the pair's binomial(1, rate), NaN where none was drawn
    step/chan_cam_xy, step/chan_tgt_xy           [T, n, 2] f64: the locations the distances were taken from
Arrays and names only are stored: data, no program text.  Every dropout and range fixture must show, per team, at least 3 delivered and at least 3
dropped messages with sender != recipient, and the NumPy verdict of tests/channel_ref.py must reproduce every recorded sent -> delivered.

    MATE_REFERENCE=<checkout of XuehaiPan/mate> python tests/golden/make_channel_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (puts the shim and the reference on sys.path, imports gym and mate)
import channel_ref as C  # noqa: E402

import mate  # noqa: E402


def channel_fixture(name, config, seed, steps, no_communication='none', range_limit=None, dropout_rate=None):
    base = mate.make('MultiAgentTracking-v0', config=config)
    base.seed(seed)
    cam_obs, tgt_obs = base.reset()
    MG.tweak_few_cargoes(base)
    cam_obs, tgt_obs = base.joint_observation()
    Nc, Nt = base.num_cameras, base.num_targets
    sizes = (Nc, Nt)

    now = {}        # this step's matrices

    def fresh():
        for team, n in enumerate(sizes):
            now['sent', team] = np.zeros((n, n), dtype=np.int8)
            now['reached', team] = np.zeros((n, n), dtype=np.int8)
            now['u', team] = np.full((n, n), np.nan)
        now['xy', 0] = np.array([[c.location[0], c.location[1]] for c in base.cameras], dtype=np.float64).reshape(Nc, 2)
        now['xy', 1] = np.array([[t.location[0], t.location[1]] for t in base.targets], dtype=np.float64).reshape(Nt, 2)
    fresh()
    ahead_of_dropout = []

    def note_sent(unwrapped, message):
        assert now['sent', message.team.value][message.sender, message.recipient] == 0      # one message per pair and step
        now['sent', message.team.value][message.sender, message.recipient] = 1
        return True

    def note_dropout_input(unwrapped, message):
        ahead_of_dropout.append(message)
        return True

    # innermost first: dropout, its recorder, the range limit, NoCommunication, the recorder of what the agents sent
    env = base
    if dropout_rate is not None:
        env = mate.MessageFilter(mate.RandomMessageDropout(env, dropout_rate), filter=note_dropout_input)
    if range_limit is not None:
        env = mate.RestrictedCommunicationRange(env, range_limit)
    if no_communication != 'none':
        env = mate.NoCommunication(env, team=no_communication)
    env = mate.MessageFilter(env, filter=note_sent)

    class_send, class_step = type(base).send_messages, type(base).step
    inside = [False]

    def send_messages(messages):
        if inside[0]:                      # the innermost wrapper: what arrives
            messages = [messages] if isinstance(messages, mate.utils.Message) else list(messages)
            for m in messages:
                now['reached', m.team.value][m.sender, m.recipient] += 1
            return class_send(base, messages)
        log = base._np_random._log         # (make_trace has installed the recording proxy: RandomMessageDropout.filter draws from env.np_random)
        before = len(log)
        del ahead_of_dropout[:]
        inside[0] = True
        try:
            env.send_messages(messages)
        finally:
            inside[0] = False
        draws = [item for item in log[before:] if item[0] == 'binomial' and item[1] == 'env']
        assert len(draws) == len(log) - before == len(ahead_of_dropout)
        for m, (_, _, _, p, u, out) in zip(ahead_of_dropout, draws):
            assert p == dropout_rate
            now['u', m.team.value][m.sender, m.recipient] = u
        del log[before:]
        return None

    rows = {key: [] for key in ('chan_cam_sent', 'chan_cam_delivered', 'chan_tgt_sent', 'chan_tgt_delivered', 'chan_cam_u', 'chan_tgt_u', 'chan_cam_xy', 'chan_tgt_xy')}

    def step(action):
        for team, tag in enumerate(('cam', 'tgt')):
            edges = np.asarray(base.communication_edges[team])
            assert np.array_equal(edges, now['reached', team]) and edges.max(initial=0) <= 1
            rows[f'chan_{tag}_sent'].append(now['sent', team])
            rows[f'chan_{tag}_delivered'].append(edges.astype(np.int8))
            rows[f'chan_{tag}_u'].append(now['u', team])
            rows[f'chan_{tag}_xy'].append(now['xy', team])
        result = class_step(base, action)
        fresh()
        return result

    base.send_messages, base.step = send_messages, step
    MG.make_trace(name, config, seed, 'greedy', steps, record_agents=True, env=base, first_obs=(cam_obs, tgt_obs))
    del base.send_messages, base.step

    path = os.path.join(HERE, name + '.npz')
    with np.load(path) as fh:
        out = {k: fh[k] for k in fh.files}
    T = len(out['step/done'])
    for key, value in rows.items():
        out['step/' + key] = np.stack(value[:T])
    out['channel/no_communication'] = np.str_(no_communication)
    out['channel/range_limit'] = np.float64(-1.0 if range_limit is None else range_limit)
    out['channel/dropout_rate'] = np.float64(0.0 if dropout_rate is None else dropout_rate)
    for key in [k for k in out if k.startswith('step/') and k[5:] in ('cam_obs', 'tgt_obs', 'state')]:
        del out[key]
    np.savez_compressed(path, **out)

    counts = []
    for team, tag in enumerate(('cam', 'tgt')):
        sent, delivered = out[f'step/chan_{tag}_sent'], out[f'step/chan_{tag}_delivered']
        n = sizes[team]
        off = ~np.eye(n, dtype=bool)[None]
        kept, dropped = int((delivered & off).sum()), int(((sent != 0) & (delivered == 0) & off).sum())
        counts.append((kept, dropped))
        disabled = no_communication in ('both', ('camera', 'target')[team])
        verdict = C.channel_verdict(disabled, out['channel/range_limit'], out['channel/dropout_rate'], None, out[f'step/chan_{tag}_u'], out[f'step/chan_{tag}_xy'])
        assert np.array_equal(delivered != 0, (sent != 0) & verdict), (name, tag)
        if dropout_rate is not None or range_limit is not None:
            assert kept >= 3 and dropped >= 3, (name, tag, kept, dropped)
    print(f'{name}: {T} steps, camera kept / dropped {counts[0]}, target kept / dropped {counts[1]}, {os.path.getsize(path) / 1024:.0f} KiB')


def main():
    MG.check_binomial_model()
    channel_fixture('channel_4v8-9_none', 'MATE-4v8-9.yaml', 3, 160, no_communication='both')
    channel_fixture('channel_4v8-9_camera_only', 'MATE-4v8-9.yaml', 3, 160, no_communication='target')
    channel_fixture('channel_4v8-9_drop30', 'MATE-4v8-9.yaml', 3, 160, dropout_rate=0.3)
    channel_fixture('channel_4v8-9_drop70', 'MATE-4v8-9.yaml', 3, 160, dropout_rate=0.7)
    channel_fixture('channel_4v8-9_range1400', 'MATE-4v8-9.yaml', 3, 160, range_limit=1400.0)
    channel_fixture('channel_8v8-9_range1000', 'MATE-8v8-9.yaml', 5, 120, range_limit=1000.0)
    channel_fixture('channel_8v8-9_range1000_drop30', 'MATE-8v8-9.yaml', 5, 120, range_limit=1000.0, dropout_rate=0.3)


if __name__ == '__main__':
    main()
