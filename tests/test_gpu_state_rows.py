"""GPU (-m gpu): the global state rows (MultiAgentTracking.state() per environment, written on the device) against the reference's
recorded traces and reset tapes, the reference's own normalisation, the observation rows of the same instant, the oracle, graph
replay, the fused rollouts and batched restarts, and the batched environment API."""
import ctypes
import os

import numpy as np
import pytest
import torch

import golden_util as G
import gpu_util as U

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
IDS = ['f64rows', 'f32rows']


def exact_columns(Nc, Nt, No):
    """Row elements that hold integers (entity counts, capacity, is_loaded / goal / empty bits, freights, bounties, cargo matrix)."""
    cols = [0, 1, 2]
    for t in range(Nt):
        base = 13 + 9 * Nc + 14 * t
        cols += [base + 3, base + 5] + list(range(base + 6, base + 14))
    tail = 13 + 9 * Nc + 14 * Nt + 3 * No
    cols += list(range(tail, tail + 2 * Nt + 16))
    return np.asarray(cols)


def check_rows(got, ref, dtype, where, exact=None):
    """The project's bars (tests/test_gpu_parity.py): f64 atol 1e-9, f32 |got - ref| <= 1e-5 max(1, |ref|); integers exact."""
    got = got.double().cpu().numpy()
    ref = np.broadcast_to(np.asarray(ref, dtype=np.float64), got.shape)
    err = np.abs(got - ref)
    print(where, 'max abs error', float(err.max()))
    if dtype == torch.float64:
        assert np.all(err <= 1e-9), (where, float(err.max()))
    else:
        assert np.all(err <= 1e-5 * np.maximum(1.0, np.abs(ref))), (where, float((err / np.maximum(1.0, np.abs(ref))).max()))
    if exact is not None:
        assert np.array_equal(got[:, exact], ref[:, exact]), (where, 'integer-valued entries')


def replay_trace(fx, dtype, normalize, ref_reset, ref_steps, steps=None):
    """Replay a reference trace (actions and tapes as test_trace_parity feeds them) on three environments with rows attached."""
    N = 3
    eng = U.engine_from_fixture(fx, N)
    Nc, Nt, No, dev = eng.num_cameras, eng.num_targets, eng.num_obstacles, eng.device
    eng.enable_state_rows(normalize=normalize, dtype=dtype)
    assert eng.state.dtype == dtype and eng.state.shape == (N, eng.state_dim)
    exact = None if normalize else exact_columns(Nc, Nt, No)
    eng.observe(tape_ct=torch.zeros((N, max(Nc, 1), Nt), dtype=torch.float64, device=dev))
    check_rows(eng.state, ref_reset, dtype, 'reset', exact)
    T = len(fx['step/done']) if steps is None else steps
    for s in range(T):
        ca = torch.from_numpy(np.broadcast_to(fx['step/cam_act'][s], (N, Nc, 2)).copy()).to(dev)
        ta = torch.from_numpy(np.broadcast_to(fx['step/tgt_act'][s], (N, Nt, 2)).copy()).to(dev)
        tape = torch.from_numpy(np.broadcast_to(np.nan_to_num(fx['step/tape_ct'][s], nan=0.0), (N, Nc, Nt)).copy()).to(dev)
        goal = torch.from_numpy(np.broadcast_to(np.nan_to_num(fx['step/goal_u'][s], nan=0.0), (N, Nt)).copy()).to(dev)
        eng.step(ca, ta, tape_ct=tape, tape_goal=goal, auto_reset=False)
        check_rows(eng.state, ref_steps[s], dtype, ('step', s), exact)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('path', G.trace_files(), ids=os.path.basename)
def test_rows_follow_the_reference_traces(path, dtype):
    """After observe() the rows are the reference's recorded reset state, after every replayed step its recorded step state."""
    fx = G.load(path)
    replay_trace(fx, dtype, False, fx['reset/state'], fx['step/state'])


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('path', G.reset_files(), ids=os.path.basename)
def test_rows_after_a_tape_reset(path, dtype):
    """reset_tape with rows attached: the launch behind the reset launches leaves the reference's post-reset state (MATE-Navigation
    included: no camera, 32 obstacles)."""
    from mate_amd.engine import Engine
    fx = G.load(path)
    cfg = G.config_of_reset_fixture(fx)
    N = 3
    eng = Engine(cfg, N, seed=5)
    Nc, Nt, No = eng.num_cameras, eng.num_targets, eng.num_obstacles
    eng.reset()
    eng.enable_state_rows(dtype=dtype)
    before = eng.state.clone()
    tape = torch.from_numpy(np.broadcast_to(fx['tape'], (N, len(fx['tape']))).copy())
    tape_ct = torch.from_numpy(np.broadcast_to(np.nan_to_num(fx['tape_ct'], nan=0.0), (N, Nc, Nt)).copy()).cuda() if Nc else None
    _, _, used = eng.reset_tape(tape, tape_ct)
    assert used.cpu().tolist() == [len(fx['tape'])] * N
    check_rows(eng.state, fx['reset/state'], dtype, 'reset_tape', exact_columns(Nc, Nt, No))
    assert not torch.equal(before, eng.state)


def _state_norm():
    return G.load('state_norm.npz')


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('name', [str(n) for n in np.load(os.path.join(G.GOLDEN_DIR, 'state_norm.npz'))['traces']]
                         if os.path.exists(os.path.join(G.GOLDEN_DIR, 'state_norm.npz')) else ['missing'])
def test_normalised_rows_equal_the_references_normalize_observation(name, dtype):
    """normalize=True against mate.normalize_observation(state, env.state_space) of the reference itself (tests/golden/state_norm.npz:
    one trace per entity shape, its first 64 steps)."""
    norm = _state_norm()
    fx = G.load(name + '.npz')
    ref_steps = norm[name + '/step']
    replay_trace(fx, dtype, True, norm[name + '/reset'], ref_steps, steps=len(ref_steps))


def _blocks_equal_observations(eng, where):
    """Every environment: camera block == camera_obs[:, c, 13:22], target block == target_obs[:, t, 13:27], counts in front."""
    N, Nc, Nt, No = eng.num_envs, eng.num_cameras, eng.num_targets, eng.num_obstacles
    row = eng.state
    counts = torch.tensor([Nc, Nt, No], dtype=row.dtype, device=row.device)
    assert torch.equal(row[:, 0:3], counts.expand(N, 3)), where
    if Nc:
        block = row[:, 13:13 + 9 * Nc].reshape(N, Nc, 9)
        assert torch.equal(block, eng.camera_obs[:, :, 13:22]), (where, 'camera block')
    block = row[:, 13 + 9 * Nc:13 + 9 * Nc + 14 * Nt].reshape(N, Nt, 14)
    assert torch.equal(block, eng.target_obs[:, :, 13:27]), (where, 'target block')


@pytest.mark.parametrize('workload,n,greedy,limit', [('MATE-4v8-9.yaml', 4096, False, None), ('MATE-8v8-9.yaml', 8192, True, None),
                                                     ('MATE-2v4-0.yaml', 16384, False, None), ('MATE-Navigation.yaml', 2048, False, None),
                                                     ('MATE-4v8-9.yaml', 515, False, 7), ('MATE-2v4-0.yaml', 16384, True, 11)])
def test_rows_show_the_same_instant_as_the_observation_rows(workload, n, greedy, limit):
    """Raw f32 rows next to f32 observations through 50 auto-resetting steps: bit for bit the agents' own private states, for ALL
    environments after every call -- a state launch ordered in front of the auto-reset launch would show a restarted environment's
    old episode.  (`limit`: a short time limit, so that every environment restarts several times.)"""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config(workload) if limit is None else read_config(workload, max_episode_steps=limit)
    eng = Engine(cfg, n, seed=17, obs_dtype=torch.float32)
    if greedy:
        eng.enable_policies()
    eng.reset()
    eng.enable_state_rows()
    _blocks_equal_observations(eng, 'reset')
    restarted = 0
    for s in range(50):
        if greedy:
            eng.step_greedy(auto_reset=True)
        else:
            eng.step_random(auto_reset=True)
        _blocks_equal_observations(eng, (workload, s))
        restarted += int((eng.scalars[:, 2] > 0).sum())
    if limit is not None:
        assert restarted >= n * (50 // (limit + 1))      # (the time limit ends an episode at its step limit + 1 at the latest)


def test_rows_against_the_oracle_at_every_step(oracle_lib):
    """MATE-4v8-9 x 256, 200 steps of external actions: f64 rows == oracle.Env.state() for every environment at every step."""
    O = oracle_lib
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    n, steps, seed, first = 256, 200, 41, 77
    threads = min(16, len(os.sched_getaffinity(0)))
    cfg = read_config('MATE-4v8-9.yaml')
    eng = Engine(cfg, n, seed=seed, first_env_index=first, obs_dtype=torch.float32)
    eng.reset()
    eng.enable_state_rows(dtype=torch.float64)
    batch = O.OracleBatch(U.oracle_proto_from_config(cfg, O), n, seed=seed, first_env_index=first)
    batch.reset(threads=threads)
    for e in range(n):
        for c in range(eng.num_cameras):
            batch.env(e).set_lut(c, *eng.lut_read(e, c))
    envs = [batch.env(e) for e in range(n)]

    def compare(where):
        ref = np.stack([env.state() for env in envs])
        err = np.abs(eng.state.cpu().numpy() - ref)
        assert np.all(err <= 1e-9), (where, float(err.max()), np.argwhere(err > 1e-9)[:4].tolist())

    compare('reset')
    rng = np.random.RandomState(3)
    for s in range(steps):
        ca = rng.uniform(-1.0, 1.0, (n, eng.num_cameras, 2)).astype(np.float32) * np.float32(6.0)
        ta = rng.uniform(-1.0, 1.0, (n, eng.num_targets, 2)).astype(np.float32) * np.float32(25.0)
        eng.step(torch.from_numpy(ca).cuda(), torch.from_numpy(ta).cuda(), auto_reset=False)
        batch.step(ca, ta, auto_reset=False, threads=threads)
        compare(s)


@pytest.mark.parametrize('versus,frame_skip,limit', [(None, 1, 9), ('camera', 1, 9), ('target', 1, 9), ('target', 5, 23)])
def test_graph_replay_refreshes_the_rows(versus, frame_skip, limit):
    """make_stepper(graph_steps=8) with rows attached: the state tensor after every replayed interval == the one an identically
    seeded engine produces with direct launches, bit for bit, across episode ends."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-4v8-9.yaml', max_episode_steps=limit)
    n = 70
    outs = []
    for graph_steps in (0, 8):
        eng = Engine(cfg, n, seed=5)
        if versus is not None:
            eng.enable_policies()
        eng.reset()
        eng.enable_state_rows()
        gen = torch.Generator(device='cuda').manual_seed(9)
        cam = (torch.rand((n, eng.num_cameras, 2), device='cuda', generator=gen) * 2 - 1) * 6
        tgt = (torch.rand((n, eng.num_targets, 2), device='cuda', generator=gen) * 2 - 1) * 25

        def policy():
            cam.mul_(-1.0).add_(0.125)
            tgt.mul_(-1.0).add_(0.25)

        stepper = eng.make_stepper(cam, tgt, auto_reset=True, graph_steps=graph_steps, between=policy, versus=versus, frame_skip=frame_skip)
        assert stepper.state is eng.state
        if not graph_steps:
            stepper.run(1)                    # the constructor's warm-up interval on the graph side
        rec = []
        for _ in range(4):
            stepper.run(8)
            torch.cuda.synchronize()
            rec.append(stepper.state.clone())
            assert torch.equal(stepper.state, eng.state_rows())      # ... and it is the state of the records as they now are
        stepper.close()
        outs.append(rec)
        del stepper, eng
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert not torch.equal(outs[0][0], outs[0][-1])


def host_state(eng, cfg):
    """state() re-assembled on the host from Engine.state_dict() (f64), in the reference's order (environment.py:894-906)."""
    sd = eng.state_dict()
    N, Nc, Nt, No = eng.num_envs, eng.num_cameras, eng.num_targets, eng.num_obstacles
    radius, theta_min, rmax, rot, zoom = U.scenario_tables(cfg)['camera'].values()      # (the order of CAMERA_DEFAULTS)
    rows = np.zeros((N, eng.state_dim))
    rows[:, 0:3] = (Nc, Nt, No)
    rows[:, 4:12] = 925.0 * np.array([1, 1, -1, 1, -1, -1, 1, -1])
    rows[:, 12] = 75.0
    j = 13
    for c in range(Nc):
        sight = np.sqrt(theta_min * rmax * rmax / sd['cam_theta'][:, c])
        phi = np.deg2rad(sd['cam_phi'][:, c])
        block = [sd['cam_x'][:, c], sd['cam_y'][:, c], np.full(N, radius), sight * np.cos(phi), sight * np.sin(phi), sd['cam_theta'][:, c],
                 np.full(N, rmax), np.full(N, rot), np.full(N, zoom)]
        rows[:, j:j + 9] = np.stack(block, axis=1)
        j += 9
    for t in range(Nt):
        cap = sd['tgt_capacity'][:, t]
        rows[:, j:j + 6] = np.stack([sd['tgt_x'][:, t], sd['tgt_y'][:, t], np.full(N, cfg['target']['sight_range']),
                                     (sd['tgt_goal_bits'][:, t] > 0).any(axis=1).astype(np.float64), cfg['target']['step_size'] / cap, cap], axis=1)
        rows[:, j + 6:j + 10] = sd['tgt_goal_bits'][:, t]
        rows[:, j + 10:j + 14] = sd['tgt_empty_bits'][:, t]
        j += 14
    for o in range(No):
        rows[:, j:j + 3] = np.stack([sd['obs_x'][:, o], sd['obs_y'][:, o], sd['obs_radius'][:, o]], axis=1)
        j += 3
    rows[:, j:j + Nt] = sd['freights']
    rows[:, j + Nt:j + 2 * Nt] = sd['bounties']
    rows[:, j + 2 * Nt:] = sd['remaining_cargoes'].reshape(N, 16)
    return rows


def test_fused_rollouts_leave_the_state_after_their_last_frame():
    """rollout_versus_greedy('target', a, 10) and rollout_random(20) with rows attached: row == on-demand rows taken right after
    == the checkpoint's fields re-assembled on the host."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-4v8-9.yaml', max_episode_steps=37)
    n = 129                                   # (129 x 220 doubles / floats: the last tile is partial; f32 rows end off a 16-byte boundary)
    for dtype in DTYPES:
        eng = Engine(cfg, n, seed=8)
        eng.enable_policies()
        eng.reset()
        eng.enable_state_rows(dtype=dtype)
        act = torch.linspace(-20.0, 20.0, n * eng.num_targets * 2, device='cuda').reshape(n, eng.num_targets, 2)
        for launch in range(6):
            before = eng.state.clone()
            if launch % 2 == 0:
                eng.rollout_versus_greedy('target', act, 10, auto_reset=True)
            else:
                eng.rollout_random(20, auto_reset=True)
            assert not torch.equal(before, eng.state)
            assert torch.equal(eng.state, eng.state_rows(dtype=dtype))
            check_rows(eng.state, host_state(eng, cfg), dtype, ('launch', launch), exact_columns(eng.num_cameras, eng.num_targets, eng.num_obstacles))
        guard = torch.full((n * eng.state_dim + 8,), -7.0, dtype=dtype, device='cuda')      # nothing is written behind the array's end
        out = guard[:n * eng.state_dim].view(n, eng.state_dim)
        eng.state_rows(out=out)
        assert torch.equal(out, eng.state) and bool((guard[n * eng.state_dim:] == -7.0).all())


def test_idle_environments_keep_their_terminal_row_until_the_batched_restart():
    """auto_reset = 4 on episodes the time limit ends in the fifth call: a finished environment's row stays its terminal row until the restart launch behind every
    fourth call, then shows the new episode."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-4v8-9.yaml', max_episode_steps=4)
    n = 33
    eng = Engine(cfg, n, seed=12)
    eng.reset()
    eng.enable_state_rows(dtype=torch.float64)
    terminal, finished_at, idle_calls = None, None, 0
    for call in range(1, 13):
        eng.step_random(auto_reset=4)
        assert torch.equal(eng.state, eng.state_rows(dtype=torch.float64))
        done = eng.scalars[:, 2].cpu().numpy()
        if terminal is None and (done == 1).all():
            terminal, finished_at = eng.state.clone(), call
        elif terminal is not None and call % 4 != 0 and call < (finished_at + 3) // 4 * 4:
            assert (done == 2).all() and torch.equal(eng.state, terminal), call
            idle_calls += 1
        elif terminal is not None and call == (finished_at + 3) // 4 * 4:
            assert bool((eng.state != terminal).any(dim=1).all()), call      # every environment restarted: new placements
            assert (eng.state_dict()['episode_step'] == 0).all()
            break
    else:
        raise AssertionError('no episode ended')
    assert finished_at % 4 != 0 and idle_calls >= 1, (finished_at, idle_calls)      # (the terminal row was seen through at least one idle call)


def test_refusals_and_detaching():
    from mate_amd._native import EngineError
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-4v8-9.yaml', max_episode_steps=40)
    n = 20
    eng = Engine(cfg, n, seed=2)
    with pytest.raises(EngineError):
        eng.enable_state_rows()                          # before the first reset
    with pytest.raises(EngineError):
        eng.state_rows()
    assert eng.state is None
    eng.enable_policies()
    eng.reset()
    buf = torch.zeros((n, eng.state_dim), dtype=torch.float32, device='cuda')
    scale = np.ones(eng.state_dim)
    for args in ((scale.ctypes.data_as(ctypes.c_void_p), None), (None, scale.ctypes.data_as(ctypes.c_void_p))):
        assert eng.lib.mate_engine_enable_state_rows(eng._h, ctypes.c_void_p(buf.data_ptr()), 0, *args) == -1       # MATE_EINVAL
        assert eng.lib.mate_engine_state_rows(eng._h, ctypes.c_void_p(buf.data_ptr()), 0, *args, eng._stream()) == -1
    assert eng.lib.mate_engine_enable_state_rows(eng._h, ctypes.c_void_p(buf.data_ptr()), 7, None, None) == -1
    assert eng.lib.mate_engine_enable_state_rows(None, ctypes.c_void_p(buf.data_ptr()), 0, None, None) == -1
    assert eng.lib.mate_engine_enable_state_rows(eng._h, ctypes.c_void_p(buf.data_ptr() + 4), 0, None, None) == -1
    eng.enable_state_rows()
    with pytest.raises(EngineError):
        eng.rollout_greedy(4, auto_reset='pipelined')
    eng.rollout_greedy(4, auto_reset=True)               # ... and the engine goes on
    # detaching restores the launch sequence: the same flows and outputs as an engine that never had rows
    outs = []
    for rows in (False, True):
        e2 = Engine(cfg, n, seed=3)
        e2.reset()
        if rows:
            e2.enable_state_rows(normalize=True)
        e2.step_random(auto_reset=True)
        if rows:
            e2.disable_state_rows()
            assert e2.state is None
        act_c = torch.full((n, e2.num_cameras, 2), 1.5, device='cuda')
        act_t = torch.full((n, e2.num_targets, 2), -7.0, device='cuda')
        e2.step(act_c, act_t, auto_reset=True)
        outs.append((e2.last_flow, [t.clone() for t in (e2.camera_obs, e2.target_obs, e2.scalars, e2.masks, e2.export_state())]))
    assert outs[0][0] == outs[1][0]
    for x, y in zip(outs[0][1], outs[1][1]):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_engine_groups_enable_rows_on_every_group():
    from mate_amd.config import read_config
    from mate_amd.engine import Engine, EngineGroups
    cfg = read_config('MATE-4v8-9.yaml')
    groups = EngineGroups(cfg, 64, groups=2, seed=6)
    groups.reset()
    states = groups.enable_state_rows(dtype=torch.float64)
    groups.each(lambda g, eng: eng.step_random(auto_reset=True))
    groups.synchronize()
    whole = Engine(cfg, 64, seed=6)
    whole.reset()
    whole.enable_state_rows(dtype=torch.float64)
    whole.step_random(auto_reset=True)
    assert torch.equal(torch.cat(states), whole.state)
    groups.close()


def test_batched_environment_state():
    """BatchedMultiAgentTracking(state_rows='normalized'): the [N, S] device tensor, inside the normalised box, == the affine map of
    a raw twin's rows."""
    from mate_amd import constants as consts
    from mate_amd.environment import BatchedMultiAgentTracking
    from mate_amd.spaces import rescale_affine
    envs = {mode: BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=64, seed=9, state_rows=mode) for mode in ('normalized', True, False)}
    for env in envs.values():
        env.reset()
        env.step_random()
    env = envs['normalized']
    state = env.state()
    assert isinstance(state, torch.Tensor) and state.is_cuda and state.shape == (64, 220) and state is env.state()
    raw_space = consts.state_space_of(4, 8, 9)
    assert np.array_equal(envs[True].state_space.low, raw_space.low) and np.array_equal(envs[True].state_space.high, raw_space.high)
    scale, bias = rescale_affine(raw_space)
    low, high = env.state_space.low, env.state_space.high
    assert np.array_equal(low, scale * raw_space.low + bias) and np.array_equal(high[np.isfinite(high)], np.ones(int(np.isfinite(high).sum())))
    got = state.double().cpu().numpy()
    assert np.all(got >= low - 1e-5) and np.all(got <= high + 1e-5)
    raw = envs[True].state()
    assert raw.shape == (64, 220)
    expect = raw.double().cpu().numpy() * scale + bias
    assert np.all(np.abs(got - expect) <= 1e-5 * np.maximum(1.0, np.abs(expect)))
    # without attached rows state() is one on-demand launch: the same rows
    assert torch.equal(envs[False].state(), raw)
    for e in envs.values():
        e.close()
