"""First rows of restarted episodes behind the fused fragments (Engine.enable_fragment_rows(first_rows=True, final_obs=True);
mate_engine_enable_first_rows): the fused K-frame flow with the feature (engine a) against the same flow without it (engine c) and against
the per-step flow with the packer's fused transform (engine b), which hands the first rows over in the call that restarts.

Bars.  Against c everything is bit-identical (the feature changes no record and no row of an environment that was not restarted).  Against b the
first rows are bit-identical for f64 rows (the operations and the order of the packer's transform on the values the plain packer wrote); for f32
the project's bar of tests/test_gpu_fragment.py, 1e-5 * max(1, |ref|), is kept as the bound.

The stagger.  Episodes last eight frames (max_episode_steps = 7).  Three held-action per-step frames, then reset(env_mask) over all of tile 0 and
every other environment of tile 1: the masked environments ("M") have eight frames left, the others ("U", all of tile 2 among them) five, so
their time limits fall into different fragments whenever a fragment is shorter than an episode: K = 1 and K = 3 restart M alone -- a proper
subset of tile 1, nothing in tile 2 -- behind one fragment and U alone behind another.  With K = 10 every environment finishes inside EVERY
fragment (eight frames, or fewer, fit into ten), whatever the stagger: there the subset condition cannot exist and the test asserts instead that
each restart takes the whole batch.  For the same reason K = 10 under the interval 2 has no restarted environment with 0 < frames < K: every
environment finishes in the interval's first fragment and idles through its second (frames = 0), behind which all of them restart.  That case
asserts frames = 0 for every restarted environment; every other case with K > 1 asserts that some restarted environment had 0 < frames < K."""
import ctypes

import pytest
import torch

from test_gpu_fragment import CASES, SENTINEL, _obs_close

pytestmark = pytest.mark.gpu
N = 40                # two full 16-environment tiles and a ragged one
TILE = 16
EPISODE_FRAMES = 8    # max_episode_steps = 7


def _stagger_mask(device):
    mask = torch.zeros(N, dtype=torch.bool, device=device)
    mask[:TILE] = True
    mask[TILE:2 * TILE:2] = True
    return mask


def _learner_rows(eng, team):
    return eng.camera_obs if team == 'camera' else eng.target_obs


def _engines(cfg, team, obs_dtype, count, seed=77):
    """`count` engines on one seed with the on-device agents, reset, then staggered: three held-action per-step frames and the masked reset."""
    from mate_amd.engine import Engine
    engines = [Engine(cfg, N, seed=seed, obs_dtype=obs_dtype) for _ in range(count)]
    agents = engines[0].num_cameras if team == 'camera' else engines[0].num_targets
    held = torch.full((N, agents, 2), 1.5, dtype=torch.float64, device=engines[0].device)
    for e in engines:
        e.enable_policies()
        e.reset()
    return engines, agents, held


def _stagger(engines, team, held):
    mask = _stagger_mask(engines[0].device)
    for e in engines:
        for _ in range(3):
            e.step_versus_greedy(team, held, auto_reset=False)
        e.reset(mask)
    return mask


def _first_rows_case(cfg, team, shaping, obs_dtype, row_dtype, K, interval, fragments=12, ragged=False):
    from mate_amd.spaces import apply_fragment_column_table, fragment_column_table
    (a, c, b), agents, held = _engines(cfg, team, obs_dtype, 3)
    if ragged:      # no compiled specialisation, and rows that are no multiple of 16 bytes: the element-wise path of both K = 1 launches
        assert not a.specialised and (agents * _learner_rows(a, team).shape[2] * _learner_rows(a, team).element_size()) % 16 != 0
    b.set_obs_transform(True, True)
    mask = _stagger((a, c, b), team, held)
    a.enable_fragment_rows(team, K, shaping=shaping, relative_coordinates=True, rescaled_observation=True, dtype=row_dtype, first_rows=True, final_obs=True)
    c.enable_fragment_rows(team, K, shaping=shaping, relative_coordinates=True, rescaled_observation=True, dtype=row_dtype)
    assert set(a.fragment) - set(c.fragment) == {'first_rows', 'first_scalars', 'final_obs'} and c.fragment_restarted is None
    assert a.fragment_final_obs.shape == a.fragment_obs.shape == a.fragment_first_rows.shape and a.fragment_first_scalars.shape == (N, 8)
    table = fragment_column_table(team, a.num_cameras, a.num_targets, a.num_obstacles, True, True)
    for e in (a, c):
        e.fragment_obs.fill_(SENTINEL)
    a.fragment_final_obs.fill_(SENTINEL)
    final_expect = a.fragment_final_obs.clone()                       # what final_obs must hold: rewritten for the restarted environments only
    gen = torch.Generator(device='cpu').manual_seed(5)
    scale = 5.0 if team == 'camera' else 20.0
    tile1, tile2 = slice(TILE, 2 * TILE), slice(2 * TILE, N)
    seen_subset = seen_early = seen_idle = seen_restart = False
    for it in range(fragments):
        act = ((torch.rand((N, agents, 2), generator=gen, dtype=torch.float64) * 2 - 1) * scale).to(a.device)
        for e in (a, c):
            e.rollout_versus_greedy(team, act, K, auto_reset=interval)
        for _ in range(K):
            b.step_versus_greedy(team, act, auto_reset=interval * K)
        torch.cuda.synchronize()
        closes = (it + 1) % interval == 0                              # b's call that has just run closes the interval: it restarts what has finished
        expect = (b.scalars[:, 2] != 0) if closes else torch.zeros(N, dtype=torch.bool, device=a.device)
        restarted = a.fragment_restarted
        print(f'fragment {it}: restarted {int(restarted.sum())} of {N}, frames of the restarted {sorted(set(a.fragment_frames[restarted].tolist()))}')
        assert torch.equal(restarted, expect), it
        # the restart's own records where it restarted, the memset's 2.0f everywhere else
        assert bool((a.fragment_first_scalars[~restarted] == 2).all()) and bool((a.fragment_first_scalars[restarted][:, 2] == 0).all()), it
        # the first rows: b's learner rows behind the call that restarted
        got, ref = a.fragment_obs[restarted], _learner_rows(b, team)[restarted]
        assert _obs_close(got, ref, obs_dtype), it
        if obs_dtype == torch.float64:
            assert torch.equal(got, ref), it
        # ... and the column table applied to the plain first rows in NumPy (the check every fragment row gets in tests/test_gpu_fragment.py)
        if bool(restarted.any()):
            again = torch.from_numpy(apply_fragment_column_table(a.fragment_first_rows[restarted].cpu().numpy(), table)).to(a.device)
            assert _obs_close(got, again, obs_dtype), it
            if obs_dtype == torch.float64:
                assert torch.equal(got, again), it
        # everything else is the flow without the feature
        assert torch.equal(a.fragment_obs[~restarted], c.fragment_obs[~restarted]), it
        final_expect[restarted] = c.fragment_obs[restarted]
        assert torch.equal(a.fragment_final_obs, final_expect), it     # (untouched rows included: the sentinel, or an earlier restart's row)
        for key in ('frames', 'done', 'rewards', 'info', 'shaped'):
            if a.fragment[key] is None:
                assert c.fragment[key] is None
            else:
                assert torch.equal(a.fragment[key], c.fragment[key]), (it, key)
        frames = a.fragment_frames
        seen_restart |= bool(restarted.any())
        if K < EPISODE_FRAMES:
            seen_subset |= bool(restarted[tile1].any()) and not bool(restarted[tile1].all()) and not bool(restarted[tile2].any())
        else:
            assert not bool(restarted.any()) or bool(restarted.all()), it
            assert interval == 1 or bool((frames[restarted] == 0).all()), it
        seen_early |= bool((restarted & (frames > 0) & (frames < K)).any())
        seen_idle |= bool((restarted & (frames == 0)).any())
    assert seen_restart
    assert seen_subset or K >= EPISODE_FRAMES          # (module docstring: no proper subset can restart once a fragment holds a whole episode)
    assert seen_early or K == 1 or (K >= EPISODE_FRAMES and interval == 2)      # (0 < frames < 1 does not exist; module docstring for K = 10, interval 2)
    assert seen_idle or interval == 1
    assert mask.any() and not mask.all()
    sa, sc = a.state_dict(), c.state_dict()
    assert set(sa) == set(sc)
    for name in sa:
        assert sa[name].tobytes() == sc[name].tobytes(), name         # bit for bit: the feature changes no record
    assert (sa['episode'] >= 2).any()


@pytest.mark.parametrize('interval', [1, 2])
@pytest.mark.parametrize('K', [1, 3, 10])
@pytest.mark.parametrize('config', list(CASES))
def test_first_rows_are_the_per_step_flows(config, K, interval):
    from mate_amd.config import read_config
    team, shaping, obs_dtype, row_dtype = CASES[config]
    _first_rows_case(read_config(config, max_episode_steps=EPISODE_FRAMES - 1), team, shaping, obs_dtype, row_dtype, K, interval)


@pytest.mark.parametrize('obs_dtype', [torch.float32, torch.float64])
def test_generic_shape_with_a_ragged_row(obs_dtype):
    """A shape without a compiled specialisation whose learner rows are no multiple of 16 bytes: the element-wise path of both K = 1 launches."""
    import shape_edges
    from mate_amd.config import read_config
    shape = (3, 5, 7)
    assert shape in [c.shape for c in shape_edges.CASES]
    cfg = read_config(shape_edges.scenario(shape), max_episode_steps=EPISODE_FRAMES - 1)
    _first_rows_case(cfg, 'target', None, obs_dtype, torch.float64, 3, 1, fragments=6, ragged=True)


def test_graph_replay():
    """Replayed fragments equal direct calls on a twin engine, first rows, final rows and restart records included, over fragments that restart."""
    from mate_amd.config import read_config
    cfg = read_config('MATE-4v8-9.yaml', max_episode_steps=EPISODE_FRAMES - 1)
    K = 3
    (a, b), agents, held = _engines(cfg, 'camera', torch.float32, 2, seed=9)
    _stagger((a, b), 'camera', held)
    for e in (a, b):
        e.enable_fragment_rows('camera', K, relative_coordinates=True, rescaled_observation=True, first_rows=True, final_obs=True)
        e.fragment_final_obs.fill_(SENTINEL)
    act = torch.zeros((N, agents, 2), dtype=torch.float64, device=a.device)
    stepper = a.make_stepper(act, None, auto_reset=1, graph_steps=2, versus='camera', frame_skip=K)
    assert stepper.fragment['final_obs'] is a.fragment_final_obs and stepper.fragment['first_scalars'] is a.fragment_first_scalars
    b.rollout_versus_greedy('camera', act, K, auto_reset=1)            # the stepper's warm-up fragment
    gen = torch.Generator(device='cpu').manual_seed(2)
    visible = 0
    for replay in range(4):
        act.copy_(((torch.rand(act.shape, generator=gen, dtype=torch.float64) * 2 - 1) * 5.0).to(a.device))
        stepper.run(2)
        for _ in range(2):
            b.rollout_versus_greedy('camera', act, K, auto_reset=1)
        torch.cuda.synchronize()
        for key in ('obs', 'final_obs', 'first_scalars', 'first_rows', 'frames', 'done', 'rewards', 'info'):
            assert torch.equal(a.fragment[key], b.fragment[key]), (replay, key)
        restarted = a.fragment_restarted
        visible += int(bool(restarted.any()))
        if bool(restarted.any()):
            assert bool((a.fragment_final_obs[restarted] != SENTINEL).any())
    assert visible >= 1                                                # a replay's last fragment restarted something
    assert bool((a.fragment_final_obs != SENTINEL).flatten(1).any(dim=1).all())      # ... and by now every environment was restarted once
    stepper.close()


def test_refusals_and_detaching():
    from mate_amd._native import MateFirstRows, MateFragmentRows
    from mate_amd.config import read_config
    cfg = read_config('MATE-4v2-9.yaml', max_episode_steps=EPISODE_FRAMES - 1)
    K = 3
    (a, c), agents, held = _engines(cfg, 'camera', torch.float32, 2, seed=3)
    lib, h = a.lib, a._h
    rows = torch.zeros((N, a.num_cameras, a.camera_obs_dim), dtype=torch.float32, device=a.device)
    final, obs = torch.zeros_like(rows), torch.zeros_like(rows)
    scalars = torch.zeros((N, 8), dtype=torch.float32, device=a.device)
    good = MateFirstRows(rows.data_ptr(), scalars.data_ptr(), final.data_ptr())
    error = lambda: lib.mate_engine_last_error().decode()  # noqa: E731
    # no fragment rows attached, or attached without obs_dev: MATE_ESTATE
    assert lib.mate_engine_enable_first_rows(h, ctypes.byref(good)) == -4 and 'fragment rows' in error()
    bare = MateFragmentRows()
    bare.team, bare.out_dtype = 0, 1
    assert lib.mate_engine_enable_fragment_rows(h, ctypes.byref(bare)) == 0
    assert lib.mate_engine_enable_first_rows(h, ctypes.byref(good)) == -4 and 'obs_dev' in error()
    bare.obs_dev = obs.data_ptr()
    assert lib.mate_engine_enable_fragment_rows(h, ctypes.byref(bare)) == 0
    # null or misaligned rows_dev / scalars_dev: MATE_EINVAL
    for bad in (MateFirstRows(None, scalars.data_ptr(), None), MateFirstRows(rows.data_ptr() + 4, scalars.data_ptr(), None),
                MateFirstRows(rows.data_ptr(), None, None), MateFirstRows(rows.data_ptr(), scalars.data_ptr() + 4, None),
                MateFirstRows(rows.data_ptr(), scalars.data_ptr(), final.data_ptr() + 2), MateFirstRows(rows.data_ptr(), scalars.data_ptr(), obs.data_ptr())):
        assert lib.mate_engine_enable_first_rows(h, ctypes.byref(bad)) == -1, error()
    assert lib.mate_engine_enable_first_rows(h, ctypes.byref(good)) == 0
    # attaching the fragment rows again for the other team detaches the first rows: that team's launches leave the buffers alone
    scalars.fill_(7.0)
    other = MateFragmentRows()
    other.team, other.out_dtype = 1, 1
    tgt_rows = torch.zeros((N, a.num_targets, a.target_obs_dim), dtype=torch.float32, device=a.device)
    other.obs_dev = tgt_rows.data_ptr()
    assert lib.mate_engine_enable_fragment_rows(h, ctypes.byref(other)) == 0
    tgt_act = torch.zeros((N, a.num_targets, 2), dtype=torch.float64, device=a.device)
    for _ in range(3):
        a.rollout_versus_greedy('target', tgt_act, K)
    torch.cuda.synchronize()
    assert bool((scalars == 7.0).all()) and bool((rows == 0).all())
    assert lib.mate_engine_enable_fragment_rows(h, None) == 0
    assert lib.mate_engine_enable_first_rows(h, ctypes.byref(good)) == -4      # (the fragment rows are gone)

    # detaching the first rows alone restores the flow without them: the terminal row is shown, over a fragment that restarts
    (a, c), agents, held = _engines(cfg, 'camera', torch.float32, 2, seed=3)      # (the target-team fragments above advanced a alone: a fresh pair)
    lib, h = a.lib, a._h
    a.enable_fragment_rows('camera', K, relative_coordinates=True, rescaled_observation=True, first_rows=True, final_obs=True)
    c.enable_fragment_rows('camera', K, relative_coordinates=True, rescaled_observation=True)
    assert a.fragment_restarted is not None
    assert lib.mate_engine_enable_first_rows(h, None) == 0
    a.fragment_first_scalars.fill_(7.0)
    act = torch.full((N, agents, 2), 2.0, dtype=torch.float64, device=a.device)
    finished = False
    for it in range(4):
        for e in (a, c):
            e.rollout_versus_greedy('camera', act, K)
        torch.cuda.synchronize()
        assert torch.equal(a.fragment_obs, c.fragment_obs) and torch.equal(a.fragment_done, c.fragment_done), it
        finished |= bool(a.fragment_done.any())
    assert finished and bool((a.fragment_first_scalars == 7.0).all()) and bool((a.fragment_final_obs == 0).all())
    # disable_fragment_rows() detaches both
    kept = a.fragment_first_scalars
    a.disable_fragment_rows()
    assert a.fragment is None and a.fragment_restarted is None and a.fragment_first_rows is None and a.fragment_final_obs is None
    a.enable_fragment_rows('camera', K, relative_coordinates=True, rescaled_observation=True)
    assert 'first_rows' not in a.fragment and a.fragment_restarted is None
    for it in range(3):
        for e in (a, c):
            e.rollout_versus_greedy('camera', act, K)
    torch.cuda.synchronize()
    assert torch.equal(a.fragment_obs, c.fragment_obs) and bool((kept == 7.0).all())


def test_batched_environment_first_rows():
    from mate_amd.environment import BatchedMultiAgentTracking
    kwargs = dict(num_envs=N, seed=4, obs_dtype=torch.float64, relative_coordinates=True, rescaled_observation=True, frame_skip=10, learner='target',
                  max_episode_steps=24)
    env = BatchedMultiAgentTracking('MATE-2v4-0.yaml', first_rows=True, **kwargs)
    plain = BatchedMultiAgentTracking('MATE-2v4-0.yaml', **kwargs)
    assert torch.equal(env.reset(), plain.reset())
    act = torch.full((N, 4, 2), 3.0, dtype=torch.float64, device=env.device)
    base = {'raw_reward', 'normalized_raw_reward', 'coverage_rate', 'real_coverage_rate', 'mean_transport_rate', 'num_delivered_cargoes', 'frames'}
    for it in range(3):                                                # 25 frames per episode: the third fragment ends on its fifth frame and restarts
        obs, rewards, done, info = env.step_fragment(act)
        obs_p, rewards_p, done_p, info_p = plain.step_fragment(act)
        torch.cuda.synchronize()
        assert set(info_p) == base and set(info) == base | {'restarted', 'final_observation'}
        eng = env.engine
        assert obs is eng.fragment_obs and info['final_observation'] is eng.fragment_final_obs
        assert torch.equal(info['restarted'], eng.fragment_restarted) and torch.equal(info['restarted'], done) and torch.equal(done, done_p)
        assert torch.equal(rewards, rewards_p) and torch.equal(info['frames'], info_p['frames'])
        restarted = info['restarted']
        assert bool(restarted.all()) == (it == 2) and bool(restarted.any()) == (it == 2)
        assert torch.equal(obs[~restarted], obs_p[~restarted])
        assert torch.equal(info['final_observation'][restarted], obs_p[restarted])
        if it == 2:
            assert not torch.equal(obs, obs_p)
    # the first rows are the rows reset() hands over: a fresh environment on the same seed whose first episode is the restarted one does not exist
    # (the episode counter enters the draws), so they are checked against the plain first rows through the column table
    from mate_amd.spaces import apply_fragment_column_table, fragment_column_table
    table = fragment_column_table('target', 2, 4, 0, True, True)
    expect = torch.from_numpy(apply_fragment_column_table(env.engine.fragment_first_rows.cpu().numpy(), table)).to(env.device)
    assert torch.equal(obs, expect)
