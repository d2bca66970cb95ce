"""GPU tests of the communication channels (mate_engine_set_channel, csrc/channel_rows.hpp: greedy_channel_kernel): the reference's own wrappers'
recorded runs replayed with their tapes (tests/golden/channel_*.npz); a permissive channel against the plain two-launch form; the four spellings of
silence; the rim of `<=`; Philox runs against their own record; sharding; batched restarts and graph replay; mixtures; the refusals.

The agents' memory has no accessor of its own: it is compared through everything it determines -- both teams' joint actions, the observation rows, the
scalars and the exported state, at every step of runs long enough for every field of it (delays, neighbours, remembered positions, warehouse sets)
to have decided an action."""
import os

import numpy as np
import pytest
import torch

import channel_ref as C
import golden_util as G
import gpu_util as U

pytestmark = pytest.mark.gpu

ESTATE, EINVAL = -4, -1
ONE_LAUNCH_FLOWS = (3, 4)      # FLOW_GREEDY / FLOW_STEP_GREEDY (csrc/engine_kernels.hpp): the agents and the step in one kernel
FIXTURES = ['channel_4v8-9_none', 'channel_4v8-9_camera_only', 'channel_4v8-9_drop30', 'channel_4v8-9_drop70', 'channel_4v8-9_range1400',
            'channel_8v8-9_range1000', 'channel_8v8-9_range1000_drop30']


def _engine(config, n, kw=None, seed=23, split=False, **more):
    """An engine with policies on, reset.  `split`: the plain two-launch form (MATE_POLICY_SPLIT is read once, at create)."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config(config, **(kw or {})) if isinstance(config, str) else config
    if split:
        os.environ['MATE_POLICY_SPLIT'] = '1'
    try:
        eng = Engine(cfg, n, seed=seed, **more)
    finally:
        os.environ.pop('MATE_POLICY_SPLIT', None)
    eng.enable_policies()
    eng.reset()
    return eng


def _plant(eng):
    from test_gpu_scripted import _plant_emptied_warehouses
    return _plant_emptied_warehouses(eng)


def _edges(eng):
    """{(team, 'sent' | 'delivered'): numpy copy}"""
    out = {}
    for team in (0, 1):
        sent, delivered = eng.channel_edges(team)
        out[team, 'sent'], out[team, 'delivered'] = sent.cpu().numpy().copy(), delivered.cpu().numpy().copy()
    return out


def _positions(sd, team):
    return np.stack([sd['cam_x'], sd['cam_y']], axis=-1) if team == 0 else np.stack([sd['tgt_x'], sd['tgt_y']], axis=-1)


def _same(a, b, what):
    assert torch.equal(a.scalars, b.scalars), what
    assert torch.equal(a.target_obs, b.target_obs), what
    assert torch.equal(a.camera_obs, b.camera_obs), what
    for x, y in zip(a.policy_actions(), b.policy_actions()):
        assert torch.equal(x, y), what


@pytest.mark.parametrize('name', FIXTURES)
def test_reference_wrappers_closed_loop(name):
    """The reference's wrappers' run replayed with the agents' and the channel's tapes: both teams' joint actions to the tolerance of the greedy
    traces (1e-8), sent / delivered exactly, at every step."""
    fx = G.load(name + '.npz')
    N = 2
    eng = U.engine_from_fixture(fx, N, obs_dtype=torch.float64)
    eng.enable_policies()
    Nc, Nt = eng.num_cameras, eng.num_targets
    dev = eng.device
    tape0 = torch.from_numpy(np.where(fx['reset/camera_target_view_mask'], 1.0, 0.0)[None].repeat(N, 0)).to(dev)
    eng.observe(tape_ct=tape0)
    no_comm, limit, rate = str(fx['channel/no_communication']), float(fx['channel/range_limit']), float(fx['channel/dropout_rate'])
    for team, tag in ((0, 'camera'), (1, 'target')):
        disabled = no_comm in ('both', tag)
        if disabled or limit >= 0 or rate > 0:
            eng.set_channel(team, disabled=disabled, range_limit=limit if limit >= 0 else None, dropout_rate=rate)
    cam_u = torch.zeros((N, Nc, Nc), dtype=torch.float64, device=dev)
    tgt_u = torch.zeros((N, Nt, Nt), dtype=torch.float64, device=dev)
    eng.channel_tape(cam_u, tgt_u)

    def bc(a, dtype=np.float64):
        a = np.asarray(a)
        return torch.from_numpy(np.broadcast_to(a, (N,) + a.shape).astype(dtype).copy()).to(dev)

    T = len(fx['step/done'])
    total = 0
    for s in range(T):
        tape = {
            'camera_resample_u': bc(np.nan_to_num(fx['step/agent_cam_binom_u'][s], nan=0.0)),
            'camera_sample_u': bc(np.nan_to_num(fx['step/agent_cam_sample_u'][s], nan=0.0)),
            'camera_delay': bc(fx['step/agent_cam_delay'][s], np.int32),
            'target_choice_u': bc(np.nan_to_num(fx['step/agent_tgt_choice_u'][s], nan=0.0)),
            'target_resample_u': bc(np.nan_to_num(fx['step/agent_tgt_binom_u'][s], nan=0.0)),
            'target_sample_u': bc(np.nan_to_num(fx['step/agent_tgt_sample_u'][s], nan=0.0)),
            'target_reset_sample_u': bc(fx['agent/tgt_reset_sample_u']),
        }
        cam_u.copy_(bc(fx['step/chan_cam_u'][s]))
        tgt_u.copy_(bc(fx['step/chan_tgt_u'][s]))
        eng.step_greedy(policy_tape=tape, tape_ct=bc(np.nan_to_num(fx['step/tape_ct'][s], nan=0.0)), tape_goal=bc(np.nan_to_num(fx['step/goal_u'][s], nan=0.0)),
                        auto_reset=False)
        cam_act, tgt_act = eng.policy_actions()
        edges = _edges(eng)
        for e in range(N):
            assert np.abs(tgt_act[e].cpu().numpy() - fx['step/tgt_act'][s]).max() < 1e-8, ('target action', s)
            assert np.abs(cam_act[e].cpu().numpy() - fx['step/cam_act'][s]).max() < 1e-8, ('camera action', s)
            for team, tag in ((0, 'cam'), (1, 'tgt')):
                assert np.array_equal(edges[team, 'sent'][e], fx[f'step/chan_{tag}_sent'][s]), (tag, 'sent', s)
                assert np.array_equal(edges[team, 'delivered'][e], fx[f'step/chan_{tag}_delivered'][s]), (tag, 'delivered', s)
        total += int(edges[0, 'sent'][0].sum()) + int(edges[1, 'sent'][0].sum())
    assert total > 0


@pytest.mark.parametrize('config,n', [('MATE-4v8-9.yaml', 96), ('MATE-2v4-0.yaml', 33), ('16v16-9', None), ('7v5-3', None), ('0v5-64', None), ('MATE-Navigation.yaml', 17)])
def test_permissive_channel_is_no_channel(config, n):
    """Rate 0, no limit, an all-ones mask, disabled=False on both teams against the plain two-launch form, 60 steps: the same bytes; sent == delivered."""
    import shape_edges
    from mate_amd.config import read_config
    if config.endswith('.yaml'):
        cfg, seeds = read_config(config, max_episode_steps=25), dict(seed=23)
    else:
        case = shape_edges.attached_case(config)
        cfg, n, seeds = dict(shape_edges.case_scenario(case), max_episode_steps=12), case.n, dict(seed=case.seed, first_env_index=case.first)
    plain, chan = _engine(cfg, n, split=True, **seeds), _engine(cfg, n, **seeds)
    if config == 'MATE-4v8-9.yaml':
        _plant(plain), _plant(chan)
    Nc, Nt = chan.num_cameras, chan.num_targets
    masks = [torch.ones((n, k, k), dtype=torch.uint8, device=chan.device) for k in (Nc, Nt)]
    for team in (0, 1):
        chan.set_channel(team, disabled=False, range_limit=None, dropout_rate=0.0, mask=masks[team])
    sent_total = 0
    for s in range(60):
        plain.step_greedy()
        chan.step_greedy()
        assert plain.last_flow not in ONE_LAUNCH_FLOWS and chan.last_flow not in ONE_LAUNCH_FLOWS
        _same(plain, chan, s)
        edges = _edges(chan)
        for team in (0, 1):
            assert np.array_equal(edges[team, 'sent'], edges[team, 'delivered']), (team, s)
            sent_total += int(edges[team, 'sent'].sum())
    assert torch.equal(plain.export_state(), chan.export_state())
    if Nc >= 2:      # (without cameras and without an emptied warehouse nobody has anything to say)
        assert sent_total > 0


def test_four_spellings_of_silence_agree():
    """disabled=True, rate 1, an all-zero mask and range_limit = 0 on both teams: the same bytes; nothing with sender != recipient arrives while
    something is sent.  (Under range_limit = 0 the copy a target's broadcast routes to its own sender arrives -- distance 0 <= 0, as in the
    reference -- and changes nothing: the three other spellings leave `delivered` all zero.)"""
    n = 48
    engines = [_engine('MATE-4v8-9.yaml', n, {'max_episode_steps': 30}) for _ in range(4)]
    for eng in engines:
        _plant(eng)
    Nc, Nt = engines[0].num_cameras, engines[0].num_targets
    zeros = [torch.zeros((n, k, k), dtype=torch.uint8, device=engines[0].device) for k in (Nc, Nt)]
    for team in (0, 1):
        engines[0].set_channel(team, disabled=True)
        engines[1].set_channel(team, dropout_rate=1.0)
        engines[2].set_channel(team, mask=zeros[team])
        engines[3].set_channel(team, range_limit=0.0)
    sent = [0, 0]
    for s in range(40):
        for eng in engines:
            eng.step_greedy()
        for k, eng in enumerate(engines):
            _same(engines[0], eng, (k, s))
            edges = _edges(eng)
            for team, size in ((0, Nc), (1, Nt)):
                off = ~np.eye(size, dtype=bool)[None]
                assert not (edges[team, 'delivered'] != 0)[np.broadcast_to(off, edges[team, 'delivered'].shape)].any(), (k, team, s)
                if k < 3:
                    assert not edges[team, 'delivered'].any(), (k, team, s)
                else:
                    assert np.array_equal(edges[team, 'delivered'] != 0, (edges[team, 'sent'] != 0) & np.eye(size, dtype=bool)[None]), (team, s)
                if k == 0:
                    sent[team] += int(edges[team, 'sent'].sum())
    assert sent[0] > 0 and sent[1] > 0


@pytest.mark.parametrize('limit,arrives', [(500.0, True), (float(np.nextafter(500.0, 0.0)), False)])
def test_rim_of_the_target_range(limit, arrives):
    """Targets 0 and 1 planted exactly 500 apart (300, 400), target 0 beside a warehouse it sees empty: its broadcast reaches target 1 at
    range_limit = 500.0 and not one place below.  Expected verdicts: tests/channel_ref.py."""
    n = 5
    eng = _engine('MATE-4v8-9.yaml', n)
    sd = eng.state_dict()
    Nt = eng.num_targets
    f = {k: np.array(sd[k], dtype=np.float64, copy=True) for k in ('tgt_x', 'tgt_y', 'tgt_empty_bits', 'remaining_cargoes', 'awaiting_cargo_counts')}
    f['tgt_x'][:, 0], f['tgt_y'][:, 0] = 100.0, 100.0
    f['tgt_x'][:, 1], f['tgt_y'][:, 1] = 400.0, 500.0
    f['tgt_empty_bits'][:] = 0
    f['tgt_empty_bits'].reshape(n, Nt, 4)[:, 0, 1] = 1
    eng.load_state_dict(f)
    eng.observe()
    eng.set_channel('target', range_limit=limit)
    sd = eng.state_dict()
    eng.step_greedy(auto_reset=False)
    edges = _edges(eng)
    expected = C.channel_verdict(False, limit, 0.0, None, np.full((n, Nt, Nt), np.nan), _positions(sd, 1))
    assert C.pair_distances(_positions(sd, 1))[0, 0, 1] == 500.0
    assert bool(expected[0, 0, 1]) == arrives
    assert (edges[1, 'sent'][:, 0, :] == 1).all() and not edges[1, 'sent'][:, 1:, :].any()
    assert np.array_equal(edges[1, 'delivered'] != 0, (edges[1, 'sent'] != 0) & expected)


@pytest.mark.parametrize('limit,arrives', [(500.0, True), (float(np.nextafter(500.0, 0.0)), False)])
def test_rim_of_the_camera_range(limit, arrives):
    """A generated scenario with two cameras fixed 500 apart (300, 400): their first messages (the 'state' every camera owes its teammates after
    reset) arrive at range_limit = 500.0 and not one place below."""
    from mate_amd.config import read_config
    base = read_config('MATE-2v4-0.yaml')
    camera = {k: v for k, v in base['camera'].items() if k not in ('location', 'location_random_range')}
    cfg = read_config(dict(base, name='MultiAgentTracking(two cameras 500 apart)', camera=dict(camera, location=[[-150.0, -200.0], [150.0, 200.0]])))
    n = 5
    eng = _engine(cfg, n)
    eng.set_channel('camera', range_limit=limit)
    sd = eng.state_dict()
    assert (C.pair_distances(_positions(sd, 0))[:, 0, 1] == 500.0).all()
    eng.step_greedy(auto_reset=False)
    edges = _edges(eng)
    expected = C.channel_verdict(False, limit, 0.0, None, np.full((n, 2, 2), np.nan), _positions(sd, 0))
    assert bool(expected[0, 0, 1]) == arrives and bool(expected[0, 1, 0]) == arrives
    assert (edges[0, 'sent'] == (1 - np.eye(2, dtype=np.int8))[None]).all()
    assert np.array_equal(edges[0, 'delivered'] != 0, (edges[0, 'sent'] != 0) & expected)


@pytest.mark.parametrize('config,n,rate', [('MATE-4v8-9.yaml', 96, 0.3), ('MATE-8v8-9.yaml', 65, 0.7)])
def test_philox_runs_against_their_own_record(config, n, rate):
    """record=True: delivered == sent & verdict(recorded u, positions, settings) at every step; a uniform is recorded exactly where a message was sent;
    the kept fraction lies within four binomial standard deviations of 1 - rate (range limit off for that count: cameras only dropout)."""
    eng = _engine(config, n, {'max_episode_steps': 40})
    if config == 'MATE-4v8-9.yaml':
        _plant(eng)
    limits = (None, 1200.0)
    for team in (0, 1):
        eng.set_channel(team, dropout_rate=rate, range_limit=limits[team])
    records = eng.channel_tape(record=True)
    kept = drawn = 0
    for s in range(80):
        sd = eng.state_dict()
        live = sd['done'] == 0
        eng.step_greedy(auto_reset=4)
        edges = _edges(eng)
        for team in (0, 1):
            u = records[team].cpu().numpy()
            sent, delivered = edges[team, 'sent'][live] != 0, edges[team, 'delivered'][live] != 0
            assert np.array_equal(np.isfinite(u[live]), sent), (team, s)
            assert ((u[live][sent] >= 0.0) & (u[live][sent] < 1.0)).all()
            verdict = C.channel_verdict(False, limits[team], rate, None, u[live], _positions(sd, team)[live])
            assert np.array_equal(delivered, sent & verdict), (team, s)
            if team == 0:
                kept += int(delivered.sum()); drawn += int(sent.sum())
    assert drawn > 200
    sigma = np.sqrt(rate * (1.0 - rate) / drawn)
    assert abs(kept / drawn - (1.0 - rate)) <= 4.0 * sigma, (kept, drawn)


def test_sharding_is_invisible():
    """Two engines over the halves (first_env_index) equal one engine over the whole batch, byte for byte: the draws are keyed by the global index."""
    whole = _engine('MATE-4v8-9.yaml', 64, {'max_episode_steps': 30}, seed=7)
    halves = [_engine('MATE-4v8-9.yaml', 32, {'max_episode_steps': 30}, seed=7, first_env_index=first) for first in (0, 32)]
    for eng in [whole] + halves:
        for team in (0, 1):
            eng.set_channel(team, dropout_rate=0.3, range_limit=1400.0)
    for s in range(50):
        for eng in [whole] + halves:
            eng.step_greedy()
        for k, half in enumerate(halves):
            span = slice(32 * k, 32 * k + 32)
            assert torch.equal(whole.scalars[span], half.scalars), s
            assert torch.equal(whole.target_obs[span], half.target_obs) and torch.equal(whole.camera_obs[span], half.camera_obs), s
            we, he = _edges(whole), _edges(half)
            for key in we:
                assert np.array_equal(we[key][span], he[key]), (key, s)


def test_batched_restart_keeps_idle_rows():
    """auto_reset = 4: an environment that has finished and waits for the batched restart is skipped by the agents' launch and keeps its edge rows."""
    eng = _engine('MATE-4v8-9.yaml', 48, {'max_episode_steps': 10})
    for team in (0, 1):
        eng.set_channel(team, dropout_rate=0.3)
    idle_seen = 0
    for s in range(40):
        done = eng.state_dict()['done'] != 0
        before = _edges(eng)
        eng.step_greedy(auto_reset=4)
        after = _edges(eng)
        idle_seen += int(done.sum())
        for key in before:
            assert np.array_equal(before[key][done], after[key][done]), (key, s)
    assert idle_seen > 0


@pytest.mark.parametrize('versus', ['camera', 'target'])
def test_stepper_graph_replays_the_channel(versus):
    """A Stepper graph (batched restarts inside it) against the same calls made directly, channels on both teams: the same bytes, the same edge rows."""
    n, K = 64, 4
    direct, graphed = (_engine('MATE-4v8-9.yaml', n, {'max_episode_steps': 14}, seed=5) for _ in range(2))
    team = 0 if versus == 'camera' else 1
    agents = (direct.num_cameras, direct.num_targets)[team]
    gen = torch.Generator(device='cpu').manual_seed(3)
    action = ((torch.rand((n, agents, 2), generator=gen) * 2.0 - 1.0) * 3.0).to(direct.device)
    for eng in (direct, graphed):
        for t in (0, 1):
            eng.set_channel(t, dropout_rate=0.3, range_limit=1400.0)
    mine = action.clone()
    stepper = graphed.make_stepper(mine if team == 0 else None, mine if team == 1 else None, auto_reset=K, graph_steps=K, versus=versus)
    stepper.run(6 * K)
    torch.cuda.synchronize()
    for s in range(stepper.warmup_steps + 6 * K):
        direct.step_versus_greedy(versus, action, auto_reset=K)
    assert direct.last_flow not in ONE_LAUNCH_FLOWS
    assert torch.equal(direct.scalars, graphed.scalars) and torch.equal(direct.target_obs, graphed.target_obs) and torch.equal(direct.camera_obs, graphed.camera_obs)
    de, ge = _edges(direct), _edges(graphed)
    for key in de:
        assert np.array_equal(de[key], ge[key]), key
    stepper.close()


@pytest.mark.parametrize('versus', ['camera', 'target'])
def test_channel_of_the_callers_team_is_inert(versus):
    """step_versus_greedy with the channel on the caller's own team: the one-launch flow, the bytes of no channel."""
    n = 64
    plain, chan = (_engine('MATE-4v8-9.yaml', n, {'max_episode_steps': 20}, seed=9) for _ in range(2))
    chan.set_channel(versus, disabled=True)
    team = 0 if versus == 'camera' else 1
    gen = torch.Generator(device='cpu').manual_seed(4)
    for s in range(30):
        action = ((torch.rand((n, (plain.num_cameras, plain.num_targets)[team], 2), generator=gen) * 2.0 - 1.0) * 3.0).to(plain.device)
        plain.step_versus_greedy(versus, action)
        chan.step_versus_greedy(versus, action)
        assert chan.last_flow == plain.last_flow and chan.last_flow in ONE_LAUNCH_FLOWS
        _same(plain, chan, s)


def test_mixture_under_a_target_channel():
    """A target mixture of {greedy, heuristic, naive} under a target channel runs; environments whose episode drew 'naive' show no `sent`."""
    import scripted_ref as R
    n = 96
    eng = _engine('MATE-4v8-9.yaml', n, {'max_episode_steps': 15})
    _plant(eng)
    eng.set_opponent_mixture('target', {'greedy': 1.0, 'heuristic': 1.0, 'naive': 1.0})
    eng.set_channel('target', dropout_rate=0.3)
    record = eng.scripted_record()
    eng.scripted_tape(record=record)
    naive, talking_sent, naive_seen = R.SCRIPTED_AGENTS.index('naive'), 0, 0
    for s in range(45):
        live = eng.state_dict()['done'] == 0
        eng.step_greedy()
        assert eng.last_flow not in ONE_LAUNCH_FLOWS
        choice = record['choice'].cpu().numpy()[1]
        sent, delivered = (x.cpu().numpy() for x in eng.channel_edges('target'))
        quiet = live & (choice == naive)
        naive_seen += int(quiet.sum())
        assert not sent[quiet].any() and not delivered[quiet].any(), s
        talking_sent += int(sent[live & (choice != naive)].sum())
    assert naive_seen > 0 and talking_sent > 0


def test_refusals_change_nothing():
    from mate_amd._native import EngineError
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-4v8-9.yaml', max_episode_steps=20)
    early = Engine(cfg, 8, seed=1)
    with pytest.raises(EngineError) as err:
        early.set_channel('target', disabled=True)       # before enable_policies
    assert err.value.code == ESTATE and early.channels == [None, None]
    eng = _engine(cfg, 32, seed=1)
    twin = _engine(cfg, 32, seed=1)
    for bad in (dict(dropout_rate=-0.1), dict(dropout_rate=1.5), dict(dropout_rate=float('nan')), dict(range_limit=float('nan'))):
        with pytest.raises(ValueError):
            eng.set_channel('camera', **bad)              # Python validates before the device ...
        from mate_amd._native import MateChannel
        import ctypes
        raw = MateChannel(0, bad.get('range_limit', -1.0), bad.get('dropout_rate', 0.0), None)
        assert eng.lib.mate_engine_set_channel(eng._h, 0, ctypes.byref(raw)) == EINVAL      # ... and the library refuses the same
    assert eng.lib.mate_engine_set_channel(eng._h, 2, None) == EINVAL
    assert eng.channels == [None, None]
    eng.step_greedy(); twin.step_greedy()
    assert eng.last_flow in ONE_LAUNCH_FLOWS              # nothing was set: the one-launch flow
    _same(eng, twin, 'after refused settings')
    # the fused rollouts that would play a channelled team
    eng.set_channel('target', dropout_rate=0.3)
    before = eng.export_state().clone()
    with pytest.raises(EngineError) as err:
        eng.rollout_greedy(4)
    assert err.value.code == ESTATE and 'channel' in str(err.value)
    action = torch.zeros((32, eng.num_cameras, 2), device=eng.device)
    with pytest.raises(EngineError) as err:
        eng.rollout_versus_greedy('camera', action, 4)
    assert err.value.code == ESTATE and 'channel' in str(err.value)
    assert torch.equal(before, eng.export_state())
    with pytest.raises(ValueError) as refused:             # ... and the stepper that would be built on them
        eng.make_stepper(action, None, versus='camera', frame_skip=4)
    assert 'channel' in str(refused.value)
    eng.rollout_versus_greedy('target', torch.zeros((32, eng.num_targets, 2), device=eng.device), 2)      # the caller plays the channelled team: inert
    eng.clear_channel('target')
    # Heuristic cameras and a camera channel, in both orders, plainly and as a mixture candidate
    eng.set_channel('camera', dropout_rate=0.3)
    with pytest.raises(EngineError) as err:
        eng.set_camera_opponent('heuristic')
    assert err.value.code == ESTATE and eng.camera_agent == 'greedy'
    with pytest.raises(EngineError) as err:
        eng.set_opponent_mixture('camera', {'greedy': 1.0, 'heuristic': 1.0})
    assert err.value.code == ESTATE and eng.mixtures[0] is None
    eng.set_opponent_mixture('camera', {'greedy': 1.0, 'heuristic': 0.0})       # zero weight: not a candidate
    eng.clear_opponent_mixture('camera')
    eng.clear_channel('camera')
    eng.set_camera_opponent('heuristic')
    with pytest.raises(EngineError) as err:
        eng.set_channel('camera', dropout_rate=0.3)
    assert err.value.code == ESTATE and eng.channels[0] is None
    eng.set_channel('target', dropout_rate=0.3)              # the target team's is fine beside Heuristic cameras
    eng.step_greedy()
    eng.set_camera_opponent('greedy')
    eng.set_opponent_mixture('camera', {'naive': 1.0, 'heuristic': 1.0})
    with pytest.raises(EngineError) as err:
        eng.set_channel('camera', disabled=True)
    assert err.value.code == ESTATE and eng.channels[0] is None
