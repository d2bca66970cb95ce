"""GPU tests of the learner's messages through the team's channel (mate_engine_enable_messages / _route_messages, csrc/message_rows.hpp:
message_rows_kernel): the reference's recorded send_messages / receive_messages / step under its channel wrappers replayed (tests/golden/message_*.npz); a
matrix of shapes, widths, payload forms and addressing against tests/message_ref.py on the engine's own state; the rim of `<=`; the spellings of silence;
no channel; the Philox draws; the counts through restarts; graph replay; inertness for every stepping flow; the refusals; the facades.

Everything is compared exactly: payloads are copied, not computed."""
import ctypes

import numpy as np
import pytest
import torch

import golden_util as G
import gpu_util as U
import message_ref as R
from test_message_host import FIXTURES, channel_of_fixture

pytestmark = pytest.mark.gpu

ESTATE, EINVAL = -4, -1


def _config(config, **kw):
    import shape_edges
    from mate_amd.config import read_config
    if isinstance(config, tuple):
        return dict(shape_edges.scenario(config), **kw)
    return read_config(config, **kw)


def _engine(config, n, kw=None, seed=23, policies=True, **more):
    from mate_amd.engine import Engine
    eng = Engine(_config(config, **(kw or {})), n, seed=seed, **more)
    if policies:
        eng.enable_policies()
    eng.reset()
    return eng


def _sizes(eng):
    return eng.num_cameras, eng.num_targets


def _positions(sd, team):
    return np.stack([sd['cam_x'], sd['cam_y']], axis=-1) if team == 0 else np.stack([sd['tgt_x'], sd['tgt_y']], axis=-1)


def _read(eng, team):
    """Host copies of the team's inbox and five edge tensors."""
    out = {name: value.cpu().numpy().copy() for name, value in eng.message_edges(team).items()}
    out['inbox'] = eng.message_inbox[team].cpu().numpy().copy()
    return out


def _same(got, want, what):
    for key in want:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (what, key)


def _np_dtype(eng):
    return np.float64 if eng.obs_dtype == torch.float64 else np.float32


def _expect(eng, team, book, channel, u, sd, pairwise, live=None):
    """What one routing call of `team` must leave, from message_ref on the engine's own state `sd` (its payload and address tensors as they are)."""
    n = _sizes(eng)[team]
    payload = eng.message_payload[team].cpu().numpy()
    address = None if eng.message_address[team] is None else eng.message_address[team].cpu().numpy()
    keep = R.verdict(channel, u, _positions(sd, team), (eng.num_envs, n, n))
    inbox, sent, delivered = R.route(payload, address, pairwise, keep)
    book.update(sd['tick'], sd['episode'], delivered, live)
    return {'inbox': inbox, 'sent': sent, 'delivered': delivered, 'step_edges': book.step_edges.copy(), 'total_edges': book.total_edges.copy(),
            'agent_edges': book.agent_edges.copy()}


# ------------------------------------------------------------------ the reference's recordings
def _load_episode(eng, fx, k, tick):
    """Every environment takes the state the fixture's episode k starts from; the occlusion tables are rebuilt from it (they decide what is seen,
    not where a target goes)."""
    view = dict(fx)
    view.update({key[len(f'ep{k}/'):]: fx[key] for key in fx if key.startswith(f'ep{k}/')})
    N = eng.num_envs
    fields = {name: np.broadcast_to(v, (N,) + v.shape) for name, v in U.fixture_state(view).items()}
    fields.update(tick=np.full(N, tick), episode=np.full(N, k + 1), done=np.zeros(N))
    eng.import_state(torch.zeros((N, eng.layout.export_width), dtype=torch.float64))
    eng.load_state_dict(fields)
    eng.rebuild_luts()
    eng.observe()


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('name', sorted(FIXTURES))
def test_reference_recordings_replayed(name, dtype):
    """The reference's run replayed: the engine steps with the recorded actions and goal draws from the state each episode started from (the targets'
    positions follow the recording to 1e-9, and no recorded distance lies within 1e-6 of a range limit), the dropout draws come from the tape.  Per round
    inbox, sent and delivered, per step step_edges, agent_edges (info's two sums) and total_edges -- the device's totals are the episode's earlier steps, the
    reference's after step() include the step's own -- exactly, through the episode end and the reset."""
    from mate_amd.engine import Engine
    fx = G.load(name + '.npz')
    N, M = 2, int(fx['msg/width'])
    eng = Engine(U.config_of_fixture(fx), N, seed=0, obs_dtype=dtype)
    eng.enable_policies()
    _load_episode(eng, fx, 0, 0)
    dev, sizes = eng.device, _sizes(eng)
    tapes = [torch.zeros((N, n, n), dtype=torch.float64, device=dev) for n in sizes]
    for team in (0, 1):
        channel = channel_of_fixture(fx, team)
        if channel is not None:
            eng.set_channel(team, **channel)
        eng.enable_messages(team, M, pairwise=True, addressed=True)
    eng.message_tape(*tapes)

    def bc(a, torch_dtype):
        a = np.asarray(a)
        return torch.from_numpy(np.broadcast_to(a, (N,) + a.shape).copy()).to(device=dev, dtype=torch_dtype)

    T = len(fx['step/done'])
    previous_total = [None, None]
    for s in range(T):
        rounds = int(fx['msg/rounds'][s])
        for k in range(rounds):
            for team, tag in enumerate(('cam', 'tgt')):
                eng.message_payload[team].copy_(bc(fx[f'msg/{tag}_payload'][s, k], dtype))
                eng.message_address[team].copy_(bc(fx[f'msg/{tag}_sent'][s, k], torch.uint8))
                tapes[team].copy_(bc(fx[f'msg/{tag}_u'][s, k], torch.float64))
            eng.route_messages(round=k)
            for team, tag in enumerate(('cam', 'tgt')):
                got = _read(eng, team)
                for e in range(N):
                    assert np.array_equal(got['inbox'][e], fx[f'msg/{tag}_inbox'][s, k].astype(got['inbox'].dtype)), (tag, 'inbox', s, k)
                    assert np.array_equal(got['sent'][e], fx[f'msg/{tag}_sent'][s, k]) and np.array_equal(got['delivered'][e], fx[f'msg/{tag}_delivered'][s, k]), (tag, s, k)
        for team, tag in enumerate(('cam', 'tgt')):
            if not rounds:
                continue
            got = _read(eng, team)
            for e in range(N):
                assert np.array_equal(got['step_edges'][e], fx[f'msg/{tag}_step_edges'][s]), (tag, 'step_edges', s)
                assert np.array_equal(got['total_edges'][e] + got['step_edges'][e], fx[f'msg/{tag}_total_edges'][s]), (tag, 'total_edges', s)
                assert np.array_equal(got['total_edges'][e], 0 * got['total_edges'][e] if previous_total[team] is None else previous_total[team]), (tag, 'earlier steps', s)
                assert np.array_equal(got['agent_edges'][e, :, 0], fx[f'msg/{tag}_out'][s]) and np.array_equal(got['agent_edges'][e, :, 1], fx[f'msg/{tag}_in'][s]), (tag, s)
        eng.step(bc(fx['step/cam_act'][s], torch.float64), bc(fx['step/tgt_act'][s], torch.float64),
                 tape_goal=bc(np.nan_to_num(fx['step/goal_u'][s], nan=0.0), torch.float64), auto_reset=False)
        sd = eng.state_dict()
        assert np.abs(_positions(sd, 1) - fx['step/tgt_xy'][s][None]).max() < 1e-9, s
        assert bool(fx['step/done'][s]) == bool(sd['done'][0] != 0)
        previous_total = [fx[f'msg/{tag}_total_edges'][s] for tag in ('cam', 'tgt')]
        if fx['step/done'][s]:
            _load_episode(eng, fx, 1, s + 1)
            previous_total = [None, None]


# ------------------------------------------------------------------ shapes, widths, payload forms, addressing
SHAPES = {'MATE-4v8-9': 'MATE-4v8-9.yaml', 'MATE-2v4-0': 'MATE-2v4-0.yaml', '16v16-9': (16, 16, 9), '9v2-0': (9, 2, 0), '7v5-3': (7, 5, 3), '1v3-2': (1, 3, 2),
          '0v5-64': (0, 5, 64)}


@pytest.mark.parametrize('shape,dtype', [(name, torch.float32) for name in SHAPES] + [('MATE-4v8-9', torch.float64), ('7v5-3', torch.float64)],
                         ids=lambda v: v if isinstance(v, str) else str(v).split('.')[-1])
def test_shape_matrix_against_message_ref(shape, dtype):
    """Per shape: widths 1 (element path), 4 (one 16-byte store in f32), 6 (f32: unaligned rows; f64: 48-byte rows), 32 x per-sender / pairwise payloads x
    broadcast / addressed sending, both teams in one launch, under a channel with dropout, a range limit and a mask; the batch is no multiple of the four
    environments of a workgroup.  The payload encodes (env, sender, recipient, k): a misplaced row cannot pass."""
    n_envs = 6 if shape == '16v16-9' else 9
    eng = _engine(SHAPES[shape], n_envs, seed=41, first_env_index=3, obs_dtype=dtype)
    dev, sizes = eng.device, _sizes(eng)
    gen = torch.Generator(device='cpu').manual_seed(11)
    sd = eng.state_dict()
    teams = [team for team in (0, 1) if sizes[team] > 0]
    masks, channels = {}, {}
    for team in teams:
        n = sizes[team]
        masks[team] = (torch.rand((n_envs, n, n), generator=gen) < 0.8).to(torch.uint8).to(dev)
        eng.set_channel(team, range_limit=(700.0, 150.0)[team], dropout_rate=0.3, mask=masks[team])
        channels[team] = {'range_limit': (700.0, 150.0)[team], 'dropout_rate': 0.3, 'mask': masks[team].cpu().numpy()}
    records = eng.message_tape(record=True)
    seen = {'kept': 0, 'dropped': 0}
    for M in (1, 4, 6, 32):
        for pairwise in (False, True):
            for addressed in (False, True):
                for team in teams:
                    payload, address, _ = eng.enable_messages(team, M, pairwise=pairwise, addressed=addressed)
                    payload.copy_(torch.from_numpy(R.encoded_payload(n_envs, sizes[team], M, pairwise, _np_dtype(eng), first_env=3)))
                    if addressed:
                        address.copy_((torch.rand(address.shape, generator=gen) < 0.6).to(torch.uint8))
                    eng.message_inbox[team].fill_(-7.0)               # the launch writes the whole block
                eng.route_messages(round=M % 16)
                for team in teams:
                    got = _read(eng, team)
                    u = records[team].cpu().numpy()
                    assert np.array_equal(np.isfinite(u), got['sent'] != 0)                 # a uniform exactly where a message was sent
                    want = _expect(eng, team, R.Counts(n_envs, sizes[team]), channels[team], u, sd, pairwise)
                    _same(got, want, (M, pairwise, addressed, team))
                    seen['kept'] += int(want['delivered'].sum())
                    seen['dropped'] += int((want['sent'] - want['delivered']).sum())
    assert seen['kept'] > 0 and seen['dropped'] > 0


# ------------------------------------------------------------------ the rim, silence, no channel
@pytest.mark.parametrize('limit,arrives', [(500.0, True), (float(np.nextafter(500.0, 0.0)), False), (0.0, False)])
def test_rim_of_the_range(limit, arrives):
    """Targets 0 and 1 planted exactly 500 apart (300, 400): the message arrives at range_limit = 500.0 and not one place below; the self-edge of a
    broadcast (distance 0) arrives under range_limit = 0."""
    n = 5
    eng = _engine('MATE-4v8-9.yaml', n)
    Nt = eng.num_targets
    sd = eng.state_dict()
    f = {k: np.array(sd[k], dtype=np.float64, copy=True) for k in ('tgt_x', 'tgt_y')}
    f['tgt_x'][:, 0], f['tgt_y'][:, 0] = 100.0, 100.0
    f['tgt_x'][:, 1], f['tgt_y'][:, 1] = 400.0, 500.0
    eng.load_state_dict(f)
    eng.observe()
    sd = eng.state_dict()
    assert R.C.pair_distances(_positions(sd, 1))[0, 0, 1] == 500.0
    eng.set_channel('target', range_limit=limit)
    payload, _, _ = eng.enable_messages('target', 4)
    payload.copy_(torch.from_numpy(R.encoded_payload(n, Nt, 4, False, np.float32)))
    eng.route_messages('target')
    got = _read(eng, 1)
    _same(got, _expect(eng, 1, R.Counts(n, Nt), {'range_limit': limit}, None, sd, False), limit)
    assert (got['delivered'][:, 0, 1] == int(arrives)).all() and (got['delivered'][:, 1, 0] == int(arrives)).all()
    assert (got['delivered'][:, np.arange(Nt), np.arange(Nt)] == 1).all()                  # the self-edges
    if limit == 0.0:
        assert got['delivered'].sum() == n * Nt


def test_spellings_of_silence_and_no_channel():
    """disabled, rate 1, an all-zero mask and an all-zero address: an all-zero inbox, nothing delivered.  With no channel set delivered == sent."""
    n = 7
    eng = _engine('MATE-4v8-9.yaml', n)
    dev, sizes = eng.device, _sizes(eng)
    gen = torch.Generator(device='cpu').manual_seed(5)
    for team in (0, 1):
        payload, address, _ = eng.enable_messages(team, 6, pairwise=True, addressed=True)
        payload.copy_(torch.from_numpy(R.encoded_payload(n, sizes[team], 6, True, np.float32)))
    zeros = [torch.zeros((n, k, k), dtype=torch.uint8, device=dev) for k in sizes]
    for spelling in ({'disabled': True}, {'dropout_rate': 1.0}, {'mask': True}, {'address': True}, None):
        for team in (0, 1):
            eng.clear_channel(team)
            eng.message_address[team].fill_(1)
            eng.message_inbox[team].fill_(3.0)
            if spelling is None:
                eng.message_address[team].copy_((torch.rand(eng.message_address[team].shape, generator=gen) < 0.5).to(torch.uint8))
            elif 'address' in spelling:
                eng.message_address[team].zero_()
            elif 'mask' in spelling:
                eng.set_channel(team, mask=zeros[team])
            else:
                eng.set_channel(team, **spelling)
        eng.route_messages()
        for team in (0, 1):
            got = _read(eng, team)
            if spelling is None:
                assert np.array_equal(got['delivered'], got['sent']) and got['sent'].any() and not got['sent'].all()
                want, _, _ = R.route(eng.message_payload[team].cpu().numpy(), eng.message_address[team].cpu().numpy(), True, np.ones(got['sent'].shape, dtype=bool))
                assert np.array_equal(got['inbox'], want)
            else:
                assert not got['inbox'].any() and not got['delivered'].any(), (spelling, team)
                assert got['sent'].all() != ('address' in spelling)


# ------------------------------------------------------------------ the draws
def test_philox_key_record_and_tape(oracle_lib):
    """The recorded uniforms are philox(seed, global environment index, tick, 28, round << 12 | team << 8 | sender << 4 | recipient).x as 32-bit uniforms
    (the oracle's Philox); fed back as a tape they give the same bytes; two rounds of one tick draw differently."""
    n, seed, first = 5, 0x1234567890abcdef, 1000
    eng = _engine('MATE-4v8-9.yaml', n, seed=seed, first_env_index=first)
    sizes = _sizes(eng)
    eng.step_random(auto_reset=False)                                    # a tick other than 0
    sd = eng.state_dict()
    for team in (0, 1):
        eng.set_channel(team, dropout_rate=0.3)
        payload, _, _ = eng.enable_messages(team, 4)
        payload.copy_(torch.from_numpy(R.encoded_payload(n, sizes[team], 4, False, np.float32)))
    records = eng.message_tape(record=True)
    by_round = {}
    for round_ in (0, 9):
        eng.route_messages(round=round_)
        by_round[round_] = [r.cpu().numpy().copy() for r in records], [_read(eng, team) for team in (0, 1)]
        for team in (0, 1):
            want = R.philox_uniforms(oracle_lib.philox, seed, first, n, sd['tick'].astype(np.int64), round_, team, sizes[team])
            assert np.array_equal(by_round[round_][0][team], want), (round_, team)
    assert not np.array_equal(by_round[0][0][1], by_round[9][0][1])
    # the record of round 9 as a tape: the same bytes (the counts go on: one more delivery per delivered pair)
    eng.message_tape(*[torch.from_numpy(u).to(eng.device) for u in by_round[9][0]])
    eng.route_messages(round=3)
    for team in (0, 1):
        got, first_time = _read(eng, team), by_round[9][1][team]
        for key in ('inbox', 'sent', 'delivered'):
            assert np.array_equal(got[key], first_time[key]), (team, key)
        assert np.array_equal(got['step_edges'], first_time['step_edges'] + first_time['delivered'])


def test_dropout_rate_and_sharding():
    """Dropout 0.3 over 8192 environments x the MATE-4v8-9 pairs drops within 4 standard errors of 0.3; two engines over the halves of a batch
    (first_env_index) give the bytes of one engine over the whole."""
    n = 8192
    eng = _engine('MATE-4v8-9.yaml', n, seed=7, policies=True)
    sent = dropped = 0
    for team in (0, 1):
        eng.set_channel(team, dropout_rate=0.3)
        eng.enable_messages(team, 1)
    eng.route_messages()
    for team in (0, 1):
        edges = eng.message_edges(team)
        sent += int(edges['sent'].sum().item())
        dropped += int((edges['sent'] - edges['delivered']).sum().item())
    assert sent == n * (16 + 64)
    assert abs(dropped / sent - 0.3) <= 4.0 * np.sqrt(0.3 * 0.7 / sent), (dropped, sent)
    whole = {team: _read(eng, team) for team in (0, 1)}
    for k, first in enumerate((0, 4096)):
        half = _engine('MATE-4v8-9.yaml', 4096, seed=7, first_env_index=first)
        for team in (0, 1):
            half.set_channel(team, dropout_rate=0.3)
            half.enable_messages(team, 1)
        half.route_messages()
        for team in (0, 1):
            got = _read(half, team)
            for key in ('sent', 'delivered', 'step_edges', 'inbox'):
                assert np.array_equal(got[key], whole[team][key][first:first + 4096]), (first, team, key)


# ------------------------------------------------------------------ the counts
@pytest.mark.parametrize('auto_reset', [1, 4], ids=['immediate', 'batched'])
def test_counts_through_restarts(auto_reset):
    """Two rounds before a step give 2 in step_edges, the next tick folds them into total_edges, a restart zeroes both for the restarted environments
    only, an environment that has finished and waits for the batched restart keeps every row -- against message_ref's tag rule on the engine's own ticks,
    episodes and done flags, at every step."""
    n = 24
    eng = _engine('MATE-4v8-9.yaml', n, {'max_episode_steps': 5}, policies=False)
    sizes = _sizes(eng)
    books = [R.Counts(n, k) for k in sizes]
    for team in (0, 1):
        payload, _, _ = eng.enable_messages(team, 4)
        payload.copy_(torch.from_numpy(R.encoded_payload(n, sizes[team], 4, False, np.float32)))
    idle = folded = restarted = 0
    last = [None, None]
    for s in range(16):
        sd = eng.state_dict()
        live = sd['done'] == 0
        idle += int((~live).sum())
        for round_ in (0, 1):
            eng.route_messages(round=round_)
            for team in (0, 1):
                got = _read(eng, team)
                want = _expect(eng, team, books[team], None, None, sd, False, live)
                if last[team] is not None:                               # (what a skipped environment keeps: the inbox and the call's matrices too)
                    for key in ('inbox', 'sent', 'delivered'):
                        want[key][~live] = last[team][key][~live]
                _same(got, want, (s, round_, team))
                last[team] = got
        assert (last[1]['step_edges'][live] == 2).all()
        folded += int((last[1]['total_edges'][live] > 0).any())
        restarted += int((live & (sd['episode'] > 1) & ~(last[1]['total_edges'] > 0).any(axis=(1, 2))).sum())
        eng.step_random(auto_reset=auto_reset)
    assert folded > 0 and restarted > 0 and (idle > 0) == (auto_reset > 1)


# ------------------------------------------------------------------ graph replay, inertness
def test_stepper_graph_replays_the_router():
    """Route + step_versus_greedy replayed from a Stepper graph (between=) against the same calls made directly: the same bytes."""
    n, K = 64, 4
    direct, graphed = (_engine('MATE-4v8-9.yaml', n, {'max_episode_steps': 14}, seed=5) for _ in range(2))
    gen = torch.Generator(device='cpu').manual_seed(3)
    action = ((torch.rand((n, direct.num_cameras, 2), generator=gen) * 2.0 - 1.0) * 3.0).to(direct.device)
    for eng in (direct, graphed):
        eng.set_channel('camera', dropout_rate=0.3, range_limit=1400.0)       # the learner's own team: inert for the agents, live for its messages
        payload, _, _ = eng.enable_messages('camera', 8)
        payload.copy_(torch.from_numpy(R.encoded_payload(n, eng.num_cameras, 8, False, np.float32)))
    mine = action.clone()
    stepper = graphed.make_stepper(mine, None, auto_reset=K, graph_steps=K, versus='camera', between=lambda: graphed.route_messages('camera', 2))
    stepper.run(5 * K)
    torch.cuda.synchronize()
    for s in range(stepper.warmup_steps + 5 * K):
        direct.route_messages('camera', 2)
        direct.step_versus_greedy('camera', action, auto_reset=K)
    assert torch.equal(direct.scalars, graphed.scalars) and torch.equal(direct.target_obs, graphed.target_obs) and torch.equal(direct.camera_obs, graphed.camera_obs)
    want, got = _read(direct, 0), _read(graphed, 0)
    _same(got, want, 'graph')
    assert want['total_edges'].any() and want['delivered'].any() and not want['delivered'].all()
    stepper.close()


def test_messages_are_inert_for_every_stepping_flow():
    """Two engines, one with messages enabled and routed on the learner's team at every call: identical observations, scalars and channel_edges through
    step, step_versus_greedy, step_greedy and rollout_random."""
    n = 32
    plain, talking = (_engine('MATE-4v8-9.yaml', n, {'max_episode_steps': 9}, seed=9) for _ in range(2))
    for eng in (plain, talking):
        eng.set_channel('target', dropout_rate=0.3)
    for team in (0, 1):
        talking.enable_messages(team, 4, pairwise=True, addressed=True)[0].fill_(1.5)
    gen = torch.Generator(device='cpu').manual_seed(4)
    cam = ((torch.rand((n, plain.num_cameras, 2), generator=gen) * 2.0 - 1.0) * 3.0).to(plain.device)
    tgt = ((torch.rand((n, plain.num_targets, 2), generator=gen) * 2.0 - 1.0) * 20.0).to(plain.device)
    flows = [lambda e: e.step(cam, tgt, auto_reset=True), lambda e: e.step_versus_greedy('camera', cam), lambda e: e.step_greedy(),
             lambda e: e.step_versus_greedy('target', tgt)]
    for s in range(12):
        talking.route_messages(round=s % 16)
        for eng in (plain, talking):
            flows[s % 4](eng)
        assert torch.equal(plain.scalars, talking.scalars) and torch.equal(plain.target_obs, talking.target_obs) and torch.equal(plain.camera_obs, talking.camera_obs), s
        for team in (0, 1):
            for a, b in zip(plain.channel_edges(team), talking.channel_edges(team)):
                assert torch.equal(a, b), (s, team)
    for eng in (plain, talking):
        eng.clear_channel('target')
    talking.route_messages()
    for a, b in zip(plain.rollout_random(6), talking.rollout_random(6)):
        assert torch.equal(a, b)
    assert torch.equal(plain.export_state(), talking.export_state())
    assert talking.message_edges('target')['total_edges'].any()


# ------------------------------------------------------------------ the refusals
def test_refusals_change_nothing():
    from mate_amd._native import EngineError, MateMessageRows
    from mate_amd.engine import Engine
    n = 6
    early = Engine(_config('MATE-4v8-9.yaml'), n, seed=1)
    early.enable_messages('camera', 4)                                   # no enable_policies needed
    assert early.lib.mate_engine_route_messages(early._h, 1, 0, early._stream()) == ESTATE      # no reset so far
    eng = _engine('MATE-4v8-9.yaml', n, seed=1, policies=False)
    lib, h = eng.lib, eng._h
    payload, address, inbox = eng.enable_messages('target', 4, addressed=True)
    payload.copy_(torch.from_numpy(R.encoded_payload(n, 8, 4, False, np.float32)))
    eng.route_messages('target')
    before = _read(eng, 1)

    def cfg(width=4, payload_ptr=payload.data_ptr(), inbox_ptr=inbox.data_ptr()):
        return ctypes.byref(MateMessageRows(width, 0, payload_ptr, address.data_ptr(), inbox_ptr))
    assert lib.mate_engine_enable_messages(h, 2, cfg()) == EINVAL and lib.mate_engine_enable_messages(h, -1, None) == EINVAL      # a team that is neither
    for bad in (cfg(width=0), cfg(width=-3), cfg(payload_ptr=None), cfg(inbox_ptr=None), cfg(payload_ptr=payload.data_ptr() + 4), cfg(inbox_ptr=inbox.data_ptr() + 8)):
        assert lib.mate_engine_enable_messages(h, 1, bad) == EINVAL
    for mask, round_ in ((0, 0), (4, 0), (-1, 0), (2, -1), (2, 16)):
        assert lib.mate_engine_route_messages(h, mask, round_, eng._stream()) == EINVAL
    assert lib.mate_engine_route_messages(h, 1, 0, eng._stream()) == ESTATE and lib.mate_engine_route_messages(h, 3, 0, eng._stream()) == ESTATE      # cameras not enabled
    assert lib.mate_engine_message_edges(h, 0, None, None, None, None, None) == ESTATE and lib.mate_engine_message_edges(h, 5, None, None, None, None, None) == EINVAL
    assert lib.mate_engine_message_tape(h, ctypes.c_void_p(payload.data_ptr() + 4), None, None, None) == EINVAL
    with pytest.raises(EngineError) as err:
        eng.route_messages('camera')
    assert err.value.code == ESTATE and 'enable_messages' in str(err.value)
    with pytest.raises(ValueError):
        eng.enable_messages('target', 0)
    assert eng.message_width == [0, 4] and eng.message_payload[1] is payload and eng.message_inbox[0] is None
    torch.cuda.synchronize()
    _same(_read(eng, 1), before, 'after the refusals')
    eng.route_messages('target')                                         # the same call again: the same bytes, one more delivery per pair
    again = _read(eng, 1)
    for key in ('inbox', 'sent', 'delivered'):
        assert np.array_equal(again[key], before[key])
    assert np.array_equal(again['step_edges'], 2 * before['step_edges'])
    # a team without agents
    nobody = Engine(_config((0, 5, 3)), 4, seed=1)
    spare = torch.zeros(64, device=nobody.device)
    raw = MateMessageRows(4, 0, spare.data_ptr(), None, spare.data_ptr())
    assert nobody.lib.mate_engine_enable_messages(nobody._h, 0, ctypes.byref(raw)) == EINVAL
    with pytest.raises(ValueError):
        nobody.enable_messages('camera', 4)
    # disable: routing the team is refused again, the other team goes on
    eng.disable_messages('target')
    assert eng.message_payload == [None, None] and lib.mate_engine_route_messages(h, 2, 0, eng._stream()) == ESTATE


# ------------------------------------------------------------------ the facades
def test_batched_environment_sends_and_receives():
    from mate_amd.environment import BatchedMultiAgentTracking
    n = 6
    env = BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=n, seed=3, camera_messages=4, target_messages=6, communication_range=250.0, max_episode_steps=20)
    env.reset()
    sd = env.engine.state_dict()
    gen = torch.Generator(device='cpu').manual_seed(8)
    for team, (name, count, M) in enumerate((('camera', 4, 4), ('target', 8, 6))):
        book = R.Counts(n, count)
        per_sender = torch.from_numpy(R.encoded_payload(n, count, M, False, np.float32))
        env.send_messages(name, per_sender)                              # a broadcast, one content per sender
        inbox, delivered = env.receive_messages(name)
        keep = R.verdict({'range_limit': 250.0}, None, _positions(sd, team), (n, count, count))
        want, _, want_delivered = R.route(per_sender.numpy(), None, False, keep)
        assert np.array_equal(inbox.cpu().numpy(), want) and np.array_equal(delivered.cpu().numpy(), want_delivered)
        book.update(sd['tick'], sd['episode'], want_delivered)
        pairwise = torch.from_numpy(R.encoded_payload(n, count, M, True, np.float32))
        address = (torch.rand((n, count, count), generator=gen) < 0.5).to(torch.uint8)
        env.send_messages(name, pairwise, address=address, round=1)      # addressed, a content per pair
        inbox, delivered = env.receive_messages(name)
        want, want_sent, want_delivered = R.route(pairwise.numpy(), address.numpy(), True, keep)
        assert np.array_equal(inbox.cpu().numpy(), want) and np.array_equal(delivered.cpu().numpy(), want_delivered)
        book.update(sd['tick'], sd['episode'], want_delivered)
        edges = env.message_edges(name)
        assert tuple(edges) == R.EDGE_NAMES and np.array_equal(edges['sent'].cpu().numpy(), want_sent)
        assert np.array_equal(edges['step_edges'].cpu().numpy(), book.step_edges) and np.array_equal(edges['agent_edges'].cpu().numpy(), book.agent_edges)
        assert 0 < want_delivered.sum() < want_sent.sum()
    env.step_random()
    env.send_messages('camera', torch.zeros((n, 4, 4)))
    assert env.message_edges('camera')['total_edges'].any()             # the next tick folded the step's edges
    plain = BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=2, seed=3)
    with pytest.raises(AssertionError):
        plain.send_messages('camera', torch.zeros((2, 4, 4)))


def test_engine_groups_forward_the_calls():
    """Two groups over a batch route what one engine over the whole batch routes (the draws are keyed by the global environment index)."""
    from mate_amd.engine import EngineGroups
    n = 16
    cfg = _config('MATE-4v8-9.yaml')
    whole = _engine('MATE-4v8-9.yaml', n, seed=6)
    groups = EngineGroups(cfg, n, groups=2, seed=6, policies=True)
    groups.reset()
    values = torch.from_numpy(R.encoded_payload(n, 8, 4, False, np.float32))
    whole.set_channel('target', dropout_rate=0.3)
    groups.each(lambda g, eng: eng.set_channel('target', dropout_rate=0.3))
    whole.enable_messages('target', 4)[0].copy_(values)
    for g, (payload, address, inbox) in enumerate(groups.enable_messages('target', 4)):
        assert address is None
        payload.copy_(values[8 * g:8 * g + 8])
    records = groups.message_tape(record=True)
    whole_records = whole.message_tape(record=True)
    whole.route_messages('target', 5)
    inboxes = groups.route_messages('target', 5)
    groups.synchronize()
    torch.cuda.synchronize()
    edges = groups.message_edges('target')
    want = _read(whole, 1)
    for g in range(2):
        span = slice(8 * g, 8 * g + 8)
        assert np.array_equal(inboxes[g][0].cpu().numpy(), want['inbox'][span])
        for key in R.EDGE_NAMES:
            assert np.array_equal(edges[g][key].cpu().numpy(), want[key][span]), (g, key)
        assert np.array_equal(records[g][1].cpu().numpy(), whole_records[1].cpu().numpy()[span])
    assert 0 < want['delivered'].sum() < want['sent'].sum()
    groups.close()
