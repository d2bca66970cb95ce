"""FrameSkip fragments on the device (Engine.enable_fragment_rows / fragment_rows; csrc/fragment_rows.hpp): the reference fixtures
through the on-demand form, the fused K-frame flow with the attached launch against K per-step launches of the same Philox streams,
graph replay, the refusals, a generic shape (the kernels' resources: tests/test_kernel_resources.py).

Bars.  done, frames, num_delivered_cargoes and the last-frame info: exact.  Against the FIXTURES, reward sums and means:
K * 2^-24 * sum|term| (the scalar record is f32) + K * 2^-53 * sum|term| (np.mean / np.sum add pairwise, the launch in frame order);
observation rows: 1e-9 absolute for f64 (the packer's order of operations differs from the reference's, tests/test_fragment_host.py).
Against the PER-STEP FLOW everything is bit-identical (same operations, same order), f32 rows included; where the issue allows the
project's f32 bar, 1e-5 * max(1, |ref|), it is kept as the bound."""
import ctypes
import os

import numpy as np
import pytest
import torch

import golden_util as G
from test_fragment_host import FIXTURES, REFUSED, fragments_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TILES = 33          # two full 16-environment tiles and a partial one
SENTINEL = 12345.0


def _obs_close(got, ref, dtype):
    got, ref = got.double(), ref.double()
    if got.numel() == 0:
        return True
    if dtype == torch.float64:
        return bool((got - ref).abs().max() <= 1e-9)
    return bool(((got - ref).abs() <= 1e-5 * ref.abs().clamp(min=1.0)).all())


# ------------------------------------------------------------------ 1. the fixtures through the on-demand form
@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_through_the_on_demand_form(name):
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    fx = G.load(name + '.npz')
    K, team = int(fx['frame_skip']), str(fx['learner_team'])
    frags = fragments_of(fx)
    F, N = len(frags), N_TILES
    eng = Engine(read_config(str(fx['config_file'])), N, seed=1, obs_dtype=torch.float64)
    eng.reset()
    A, D = fx['frame/rows'].shape[1:]
    MW, W = eng.layout.mask_words, fx['frame/view_words'].shape[1]
    assert eng.layout.bit_camera_target == 0
    rows, scalars, masks = np.zeros((K, N, A, D)), np.zeros((K, N, 8), dtype=np.float32), np.zeros((K, N, MW), dtype=np.uint32)
    scalars[:, :, 2] = 2.0                                  # slots that did not run: done = 2, zero records
    which = np.arange(N) % F                                # environment n replays recorded fragment n mod F
    for n, (first, frames) in enumerate(frags[i] for i in which):
        rows[:frames, n] = fx['frame/rows'][first:first + frames]
        scalars[:frames, n] = fx['frame/scalars'][first:first + frames].astype(np.float32)
        masks[:frames, n, :W] = fx['frame/view_words'][first:first + frames]
    shaping = (dict(zip((str(k) for k in fx['aux_keys']), (float(c) for c in fx['aux_coefficients']))), str(fx['aux_reduction'])) if 'aux_keys' in fx else None
    dev = eng.device
    out = eng.fragment_rows(team, torch.from_numpy(rows).to(dev), torch.from_numpy(scalars).to(dev), torch.from_numpy(masks.view(np.int32)).to(dev),
                            shaping=shaping, relative_coordinates=True, rescaled_observation=True)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    counts = fx['skip/frames'][which]
    assert (counts < K).any() and (counts == K).any()
    assert np.array_equal(got['frames'], counts)
    assert np.array_equal(got['done'].astype(bool), fx['skip/dones'][which].all(axis=1))
    info = fx['skip/info'][which]                           # raw_reward, normalized_raw_reward | coverage_rate, real_coverage_rate | mean_transport_rate, num_delivered_cargoes
    camera = team == 'camera'
    terms = np.stack([np.abs(fx['frame/scalars'][first:first + frames]).sum(axis=0) for first, frames in (frags[i] for i in which)])     # [N, 8]: sum |term| per column
    bound = lambda col: K * (2.0 ** -24 + 2.0 ** -53) * terms[:, col]  # noqa: E731
    errors = {
        'raw_reward': (np.abs(got['rewards'][:, 0 if camera else 1] - info[:, 0]), bound(0 if camera else 1)),
        'normalized_raw_reward': (np.abs(got['rewards'][:, 3 if camera else 2] - info[:, 1]), bound(7)),
        'coverage_rate': (np.abs(got['info'][:, 0] - info[:, 2]), bound(3)),
        'real_coverage_rate': (np.abs(got['info'][:, 1] - info[:, 3]), bound(4)),
    }
    for key, (err, limit) in errors.items():
        print(f'{name} {key}: worst error {err.max():.3e}, bound there {limit[err.argmax()]:.3e}')
    for key, (err, limit) in errors.items():
        assert (err <= limit).all(), key
    assert np.array_equal(got['rewards'][:, 2], -got['rewards'][:, 3])
    assert np.array_equal(got['info'][:, 2], info[:, 4].astype(np.float32).astype(np.float64))       # last frame's mean_transport_rate, as the f32 record holds it
    assert np.array_equal(got['info'][:, 3], info[:, 5])                                            # num_delivered_cargoes: exact
    err = np.abs(got['obs'] - fx['skip/obs'][which]).max()
    print(f'{name} observation rows: worst error {err:.3e}')
    assert err <= 1e-9
    if shaping is not None:                                 # the chain's summed shaped rows: coverage_rate (f32 record) and num_tracked (integers) per frame
        expect = fx['skip/rewards'][which]
        assert set(shaping[0]) == {'coverage_rate', 'num_tracked'}
        per_fragment = abs(shaping[0]['coverage_rate']) * terms[:, 3] + abs(shaping[0]['num_tracked']) * int(fx['num_targets']) * counts      # sum |c * term|, num_tracked <= Nt
        limit = (K * (2.0 ** -24 + 2.0 ** -53) * per_fragment)[:, None]
        err = np.abs(got['shaped'] - expect)
        print(f'{name} shaped rows: worst error {err.max():.3e}, bound there {limit.max():.3e}')
        assert (err <= limit).all()
    else:                                                   # RepeatedRewardIndividualDone: the team reward per agent
        err = np.abs(got['rewards'][:, 1, None] - fx['skip/rewards'][which])
        assert (err <= bound(1)[:, None]).all()


# ------------------------------------------------------------------ 2. fused flow + attached launch == K per-step launches
CASES = {
    'MATE-2v4-0.yaml': ('target', ({'raw_reward': 1.0, 'is_tracked': -0.5, 'baseline': 0.125}, 'none'), torch.float64, torch.float64),
    'MATE-4v8-9.yaml': ('camera', ({'raw_reward': 0.5, 'coverage_rate': 1.0, 'num_tracked': 0.25}, 'mean'), torch.float64, torch.float64),
    'MATE-4v2-9.yaml': ('camera', ({'coverage_rate': 1.0, 'real_coverage_rate': -2.0, 'num_tracked': 0.5}, 'sum'), torch.float32, torch.float32),
}


@pytest.mark.parametrize('interval', [1, 2])
@pytest.mark.parametrize('K', [1, 3, 10])
@pytest.mark.parametrize('config', list(CASES))
def test_fused_fragments_are_the_per_step_flow(config, K, interval):
    _fused_case(config, K, interval, max_episode_steps=7)


@pytest.mark.parametrize('config', list(CASES))
def test_single_frame_fragments_idle_through_an_interval(config):
    """K = 1 under the restart interval 2 with max_episode_steps = 7 never idles: the eight-frame episodes end on the interval's last call.
    Seven-frame episodes (max_episode_steps = 6) end on its first call every other episode, so the second launch finds frames = 0."""
    _fused_case(config, 1, 2, max_episode_steps=6, must_idle=True)


def _fused_case(config, K, interval, max_episode_steps, must_idle=False):
    """Twelve fragments of rollout_versus_greedy + the attached launch (engine a, plain rows) against K x step_versus_greedy with the
    action held, the packer's fused transform and accumulating reward rows (engine b), restated as FrameSkip in torch f64 in frame
    order.  The batched restart `interval * K` of the per-step flow is the fused flow's restart behind every `interval`-th launch;
    interval = 2 leaves environments idle through a whole fragment (frames = 0: their rows must keep what they held).
    Observation rows: b's packer rows wherever b still holds them -- the per-step restart repacks a restarted environment's row inside
    the very call that finished it, so THOSE rows are compared with the table applied to a's own plain rows in NumPy (the check every
    row gets as well)."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    from mate_amd.spaces import apply_fragment_column_table, fragment_column_table
    team, shaping, obs_dtype, row_dtype = CASES[config]
    cfg = read_config(config, max_episode_steps=max_episode_steps)
    N = N_TILES
    a, b = (Engine(cfg, N, seed=77, obs_dtype=obs_dtype) for _ in range(2))
    b.set_obs_transform(True, True)
    for e in (a, b):
        e.enable_policies()
        e.reset()
    a.enable_fragment_rows(team, K, shaping=shaping, relative_coordinates=True, rescaled_observation=True, dtype=row_dtype)
    b.enable_reward_rows(**{team: shaping}, dtype=row_dtype, accumulate=True)
    b_rows = b.camera_reward_rows if team == 'camera' else b.target_reward_rows
    table = fragment_column_table(team, a.num_cameras, a.num_targets, a.num_obstacles, True, True)
    agents = a.num_cameras if team == 'camera' else a.num_targets
    a.fragment_obs.fill_(SENTINEL)
    gen = torch.Generator(device='cpu').manual_seed(5)
    code = 0 if team == 'camera' else 1
    seen_idle = seen_early = False
    for it in range(12):
        scale = 5.0 if team == 'camera' else 20.0
        act = ((torch.rand((N, agents, 2), generator=gen, dtype=torch.float64) * 2 - 1) * scale).to(a.device)
        before = a.fragment_obs.clone()
        cam, tgt, sc = a.rollout_versus_greedy(team, act, K, auto_reset=interval)
        plain = (cam if team == 'camera' else tgt).clone()
        # the per-step flow and FrameSkip restated
        frames = torch.zeros(N, dtype=torch.int32, device=a.device)
        done = torch.zeros(N, dtype=torch.bool, device=a.device)
        sums, cov = torch.zeros((N, 3), dtype=torch.float64, device=a.device), torch.zeros((N, 2), dtype=torch.float64, device=a.device)
        last = torch.zeros((N, 2), dtype=torch.float64, device=a.device)
        obs, held = torch.zeros_like(a.fragment_obs), torch.zeros(N, dtype=torch.bool, device=a.device)
        b_rows.zero_()
        for f in range(K):
            b.step_versus_greedy(team, act, auto_reset=interval * K)
            s = b.scalars.double()
            live = s[:, 2] != 2
            assert torch.equal(sc[f][:, :3], b.scalars[:, :3]), (it, f)
            frames += live.int()
            done |= live & (s[:, 2] == 1)
            sums += torch.where(live[:, None], s[:, [0, 1, 7]], torch.zeros_like(sums))
            cov += torch.where(live[:, None], s[:, [3, 4]], torch.zeros_like(cov))
            last = torch.where(live[:, None], s[:, [5, 6]], last)
            rows = b.camera_obs if team == 'camera' else b.target_obs
            restarted = live & (s[:, 2] == 1) & ((it * K + f + 1) % (interval * K) == 0)      # b repacked these rows behind the step
            obs = torch.where((live & ~restarted)[:, None, None], rows, obs)
            held = (held | live) & ~restarted
        torch.cuda.synchronize()
        assert torch.equal(a.fragment_frames, frames), it
        assert torch.equal(a.fragment_done.bool(), done), it
        assert torch.equal(a.fragment_rewards[:, :3], sums) and torch.equal(a.fragment_rewards[:, 3], -sums[:, 2]), it
        ran = frames > 0
        means = torch.where(ran[:, None], cov / frames.clamp(min=1).double()[:, None], torch.zeros_like(cov))
        assert torch.equal(a.fragment_info[:, :2], means) and torch.equal(a.fragment_info[:, 2:], last), it
        assert torch.equal(a.fragment_shaped, b_rows), it
        got = a.fragment_obs
        assert torch.equal(got[~ran], before[~ran]), it                       # frames = 0: untouched
        assert _obs_close(got[held], obs[held], obs_dtype), it
        if obs_dtype == torch.float64:
            assert torch.equal(got[held], obs[held]), it
        last_frame = torch.zeros(N, dtype=torch.long, device=a.device)
        for f in range(K):
            last_frame = torch.where(sc[f][:, 2] != 2, torch.full_like(last_frame, f), last_frame)
        picked = plain[last_frame, torch.arange(N, device=a.device)].cpu().numpy()
        expect = torch.from_numpy(apply_fragment_column_table(picked, table)).to(a.device)
        assert _obs_close(got[ran], expect[ran], obs_dtype), it
        if obs_dtype == torch.float64:
            assert torch.equal(got[ran], expect[ran]), it
        seen_idle |= bool((~ran).any())
        seen_early |= bool((ran & (frames < K)).any())
    assert (a.state_dict()['episode'] >= 2).any()
    assert seen_early or K == 1
    assert seen_idle or interval == 1 or (K == 1 and not must_idle)      # (K = 1, eight-frame episodes: they end on the interval's last call and restart at once)
    if interval == 2:
        assert (a.fragment_obs != SENTINEL).any()


# ------------------------------------------------------------------ 3. graph replay
def test_graph_replay_and_coefficients_in_place():
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-4v8-9.yaml', max_episode_steps=7)
    N, K = N_TILES, 5
    shaping = ({'coverage_rate': 1.0, 'num_tracked': 0.25}, 'mean')
    engines = []
    for _ in range(3):
        e = Engine(cfg, N, seed=9, obs_dtype=torch.float32)
        e.enable_policies()
        e.reset()
        e.enable_fragment_rows('camera', K, shaping=shaping, relative_coordinates=True, rescaled_observation=True)
        engines.append(e)
    a, b, c = engines                                                  # graph-replayed | launched directly | launched directly, coefficients never rewritten
    act = torch.zeros((N, a.num_cameras, 2), dtype=torch.float64, device=a.device)
    gen = torch.Generator(device='cpu').manual_seed(2)
    stepper = a.make_stepper(act, None, auto_reset=1, graph_steps=2, versus='camera', frame_skip=K)
    assert stepper.fragment['obs'] is a.fragment_obs
    for e in (b, c):
        e.rollout_versus_greedy('camera', act, K, auto_reset=1)         # the stepper's warm-up fragment
    changed = None
    for replay in range(3):
        act.copy_(((torch.rand(act.shape, generator=gen, dtype=torch.float64) * 2 - 1) * 5.0).to(a.device))
        if replay == 2:                                                  # a schedule: rewritten in place between two replays
            for e in (a, b):
                e.fragment_coefficients[1] = 3.0
            changed = True
        stepper.run(2)
        for _ in range(2):
            for e in (b, c):
                e.rollout_versus_greedy('camera', act, K, auto_reset=1)
        torch.cuda.synchronize()
        for key in ('obs', 'rewards', 'done', 'frames', 'info', 'shaped'):
            assert torch.equal(a.fragment[key], b.fragment[key]), (replay, key)
    assert changed
    # the rewritten coefficient took effect: everything but the shaped rows equals the engine that kept coefficient 1, and the shaped rows
    # exceed its rows by 2 * sum(coverage_rate) -- sums of at most K f64 terms below 8 each: 1e-12 covers their rounding many times over
    for key in ('obs', 'rewards', 'done', 'frames', 'info'):
        assert torch.equal(a.fragment[key], c.fragment[key]), key
    extra = 2.0 * a.fragment_info[:, 0] * a.fragment_frames.double()
    covered = extra > 0                                                  # (an environment that covered nothing gains nothing)
    assert bool(covered.any()) and bool((a.fragment_shaped[covered] != c.fragment_shaped[covered]).all())
    assert float((a.fragment_shaped - c.fragment_shaped - extra[:, None]).abs().max()) <= 1e-12
    stepper.close()


# ------------------------------------------------------------------ 4. refusals and hygiene
@pytest.mark.parametrize('key', REFUSED)
def test_state_dependent_terms_give_einval(key):
    from mate_amd._native import EngineError
    from mate_amd.config import read_config
    from mate_amd.engine import Engine, reward_term_keys
    eng = Engine(read_config('MATE-4v2-9.yaml'), 8, seed=1)
    eng.reset()
    for team in ('camera', 'target'):
        if key not in reward_term_keys(team):
            continue
        with pytest.raises(EngineError, match=key) as info:
            eng.enable_fragment_rows(team, 3, shaping=({key: 0.5}, 'none'))
        assert info.value.code == -1                       # MATE_EINVAL
        assert eng.fragment is None


def test_error_paths_and_detach():
    from mate_amd._native import EngineError, MateFragmentRows
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    eng = Engine(read_config('MATE-4v2-9.yaml'), 8, seed=1)
    eng.enable_policies()
    with pytest.raises(EngineError, match='before reset') as info:
        eng.enable_fragment_rows('camera', 3)
    assert info.value.code == -4                           # MATE_ESTATE
    eng.reset()
    act = torch.zeros((8, eng.num_cameras, 2), dtype=torch.float64, device=eng.device)
    eng.rollout_versus_greedy('camera', act, 3)
    flow_before = eng.last_flow
    cfg = MateFragmentRows()
    cfg.team = 2
    assert eng.lib.mate_engine_enable_fragment_rows(eng._h, ctypes.byref(cfg)) == -1 and 'team' in eng.lib.mate_engine_last_error().decode()
    cfg.team, cfg.out_dtype = 0, 7
    assert eng.lib.mate_engine_enable_fragment_rows(eng._h, ctypes.byref(cfg)) == -1 and 'out_dtype' in eng.lib.mate_engine_last_error().decode()
    cfg.out_dtype, cfg.reduction = 1, 9
    assert eng.lib.mate_engine_enable_fragment_rows(eng._h, ctypes.byref(cfg)) == -1 and 'reduction' in eng.lib.mate_engine_last_error().decode()
    buf = torch.zeros(64, dtype=torch.float64, device=eng.device)
    cfg.reduction, cfg.rewards_dev = 0, buf.data_ptr() + 4
    assert eng.lib.mate_engine_enable_fragment_rows(eng._h, ctypes.byref(cfg)) == -1 and 'aligned' in eng.lib.mate_engine_last_error().decode()
    cfg.rewards_dev, cfg.shaped_dev = None, buf.data_ptr()
    assert eng.lib.mate_engine_enable_fragment_rows(eng._h, ctypes.byref(cfg)) == -1 and 'coefficient' in eng.lib.mate_engine_last_error().decode()
    nav = Engine(read_config('MATE-Navigation.yaml'), 8, seed=1)
    nav.reset()
    with pytest.raises(EngineError, match='no cameras') as info:
        nav.enable_fragment_rows('camera', 3)
    assert info.value.code == -1

    eng.enable_fragment_rows('camera', 3, shaping=({'num_tracked': 1.0}, 'none'))
    with pytest.raises(EngineError, match='pipelined') as info:
        eng.rollout_greedy(2, auto_reset='pipelined')
    assert info.value.code == -4
    eng.rollout_versus_greedy('camera', act, 3)
    torch.cuda.synchronize()
    assert int(eng.fragment_frames.min()) == 3
    # the other team's launches and the per-step flow do not enqueue it
    frames = eng.fragment_frames
    frames.fill_(-1)
    tgt_act = torch.zeros((8, eng.num_targets, 2), dtype=torch.float64, device=eng.device)
    eng.rollout_versus_greedy('target', tgt_act, 3)
    eng.step_versus_greedy('camera', act)
    eng.disable_fragment_rows()
    assert eng.fragment is None and eng.fragment_obs is None
    eng.rollout_versus_greedy('camera', act, 3)            # detached: today's launch list
    eng.rollout_greedy(2, auto_reset='pipelined')
    torch.cuda.synchronize()
    eng.rollout_versus_greedy('camera', act, 3)
    torch.cuda.synchronize()
    assert int(frames.max()) == -1
    assert eng.last_flow == flow_before                  # the same kernel form as before anything was attached


# ------------------------------------------------------------------ 5. a generic shape, rows that are no multiple of 16 bytes
@pytest.mark.parametrize('obs_dtype', [torch.float32, torch.float64])
def test_generic_shape_with_a_ragged_row(obs_dtype):
    import shape_edges
    from mate_amd.engine import Engine
    from mate_amd.spaces import apply_fragment_column_table, fragment_column_table
    shape = (3, 5, 7)
    assert shape in [c.shape for c in shape_edges.CASES]
    N, K = N_TILES, 3
    eng = Engine(shape_edges.scenario(shape), N, seed=3, obs_dtype=obs_dtype)
    assert not eng.specialised
    eng.reset()
    A, D = eng.num_targets, eng.target_obs_dim
    assert (A * D * (4 if obs_dtype == torch.float32 else 8)) % 16 != 0
    rows, scalars = [], []
    for f in range(K):
        eng.step_random(auto_reset=False)
        rows.append(eng.target_obs.clone())
        scalars.append(eng.scalars.clone())
    rows, scalars = torch.stack(rows), torch.stack(scalars)
    last = torch.arange(N, device=eng.device) % (K + 1) - 1            # -1: no frame ran; else the last live frame
    for f in range(K):
        scalars[f, :, 2] = torch.where(last >= f, torch.zeros(N, device=eng.device), torch.full((N,), 2.0, device=eng.device))
    ran = last >= 0
    picked = rows[last.clamp(min=0), torch.arange(N, device=eng.device)]
    out = {'obs': torch.full((N, A, D), SENTINEL, dtype=obs_dtype, device=eng.device), 'frames': torch.zeros(N, dtype=torch.int32, device=eng.device)}
    eng.fragment_rows('target', rows, scalars, out=out)                 # a plain copy: a gather
    torch.cuda.synchronize()
    assert torch.equal(out['frames'].long(), last + 1)
    assert torch.equal(out['obs'][ran], picked[ran]) and bool((out['obs'][~ran] == SENTINEL).all())
    table = fragment_column_table('target', *shape, relative_coordinates=True, rescaled_observation=True)
    eng.fragment_rows('target', rows, scalars, out=out, relative_coordinates=True, rescaled_observation=True)
    torch.cuda.synchronize()
    expect = torch.from_numpy(apply_fragment_column_table(picked.cpu().numpy(), table)).to(eng.device)
    assert _obs_close(out['obs'][ran], expect[ran], obs_dtype) and bool((out['obs'][~ran] == SENTINEL).all())


def test_batched_environment_fragments():
    """BatchedMultiAgentTracking(frame_skip=K, learner=...): reset() returns the transformed rows (the per-step packer's, bit for bit),
    step_fragment the reduced fragment; unshaped rewards are the team reward per agent."""
    from mate_amd.environment import BatchedMultiAgentTracking
    env = BatchedMultiAgentTracking('MATE-2v4-0.yaml', num_envs=N_TILES, seed=4, obs_dtype=torch.float64, relative_coordinates=True,
                                    rescaled_observation=True, frame_skip=10, learner='target', max_episode_steps=24)
    ref = BatchedMultiAgentTracking('MATE-2v4-0.yaml', num_envs=N_TILES, seed=4, obs_dtype=torch.float64, relative_coordinates=True,
                                    rescaled_observation=True, max_episode_steps=24)
    ref.enable_greedy_policies()
    obs = env.reset()
    assert obs.shape == (N_TILES, 4, env.engine.target_obs_dim) and torch.equal(obs, ref.reset()[1])
    act = torch.full((N_TILES, 4, 2), 3.0, dtype=torch.float64, device=env.device)
    total = 0
    for _ in range(3):
        obs, rewards, done, info = env.step_fragment(act)
        torch.cuda.synchronize()
        assert rewards.shape == (N_TILES, 4) and torch.equal(rewards[:, 0], info['raw_reward']) and torch.equal(rewards[:, 0], rewards[:, 3])
        total += int(info['frames'].sum())
        assert set(info) == {'raw_reward', 'normalized_raw_reward', 'coverage_rate', 'real_coverage_rate', 'mean_transport_rate', 'num_delivered_cargoes', 'frames'}
    assert bool(done.all()) and total == N_TILES * 25      # 25 frames per episode: the third fragment ends on its fifth frame
    # a masked reset repacks the listed environments only: the other rows stay what the last fragment left
    from mate_amd.spaces import apply_fragment_column_table, fragment_column_table
    before = obs.clone()
    mask = torch.zeros(N_TILES, dtype=torch.bool, device=env.device)
    mask[[0, 17, 32]] = True
    after = env.reset(mask)
    torch.cuda.synchronize()
    assert torch.equal(after[~mask], before[~mask]) and not torch.equal(after[mask], before[mask])
    table = fragment_column_table('target', 2, 4, 0, True, True)
    expect = torch.from_numpy(apply_fragment_column_table(env.engine.target_obs[mask].cpu().numpy(), table)).to(env.device)
    assert torch.equal(after[mask], expect)
