"""Per-frame FrameSkip fragments on the device (Engine.enable_fragment_rows(per_frame=True); csrc/frame_rows.hpp):
the recorded fixtures through the on-demand form, the Greedy opponents against the fused fragment of section 3.9, the other opponents and
the four state-dependent shaping terms against a twin engine stepped per frame and reduced in NumPy (tests/frame_fragment_ref.py), graph
replay, inertness, the stack of attachments, refusals and facades.

Bars.  Fixtures: those tests/test_gpu_fragment.py derives (frame_fragment_ref.check_fixture).  Everything else is bit for bit: the frame
launch makes the fused fragment's f64 adds in its order, and the twin's reduction is the same operations in NumPy.  One exception is
stated where it applies: the twin's restart repacks a row inside the call that finished it, so the terminal row of an environment that
ends on a fragment's closing frame exists only in the attached engine (its final_obs row is then not compared)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import frame_fragment_ref as R
import golden_util as G
from test_fragment_host import FIXTURES
from test_gpu_fragment import CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TILES = 33          # two full 16-environment tiles and a partial one
KEYS = ('obs', 'rewards', 'done', 'frames', 'info', 'shaped')


def _same(a, b):
    """Bit for bit: equal as bytes, or equal values of one type (a zero's sign apart)."""
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a, b))


def _actions(gen, N, agents, team, device):
    scale = 5.0 if team == 'camera' else 20.0
    return ((torch.rand((N, agents, 2), generator=gen, dtype=torch.float64) * 2 - 1) * scale).to(device)


# ------------------------------------------------------------------ 1. the fixtures through the on-demand form
@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_through_the_on_demand_form(name):
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    fx = G.load(name + '.npz')
    K, team = int(fx['frame_skip']), str(fx['learner_team'])
    N = 37
    eng = Engine(read_config(str(fx['config_file'])), N, seed=1, obs_dtype=torch.float64)
    eng.reset()
    rows, scalars, which = R.fixture_frames(fx, N)
    rows, scalars = torch.from_numpy(rows).to(eng.device), torch.from_numpy(scalars).to(eng.device)
    out = None
    for f in range(K):
        out = eng.frame_fragment(team, rows[f], scalars[f], f, K, out=out)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    R.check_fixture(name, got, fx, which)
    # and the NumPy restatement, bit for bit
    st = R.new_state(N, *rows.shape[2:])
    for f in range(K):
        R.fold_frame(st, scalars[f].cpu().numpy(), rows[f].cpu().numpy(), f, K)
    for key in ('obs', 'rewards', 'info', 'done', 'frames'):
        assert np.array_equal(got[key], st[key]), key


# ------------------------------------------------------------------ 2. Greedy opponents: the fused fragment, bit for bit
def _against_fused(config, K, interval, max_episode_steps, must_idle=False, fragments=12):
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    team, shaping, obs_dtype, row_dtype = CASES[config]
    cfg = read_config(config, max_episode_steps=max_episode_steps)
    N = N_TILES
    a, b = (Engine(cfg, N, seed=77, obs_dtype=obs_dtype) for _ in range(2))
    for e in (a, b):
        e.enable_policies()
        e.reset()
    common = dict(shaping=shaping, relative_coordinates=True, rescaled_observation=True, dtype=row_dtype, first_rows=True, final_obs=True)
    a.enable_fragment_rows(team, K, **common)
    b.enable_fragment_rows(team, K, per_frame=True, **common)
    assert set(b.fragment) >= set(KEYS) | {'restarted', 'final_obs'}
    agents = a.num_cameras if team == 'camera' else a.num_targets
    gen = torch.Generator(device='cpu').manual_seed(5)
    seen_idle = seen_early = seen_restart = False
    for it in range(fragments):
        act = _actions(gen, N, agents, team, a.device)
        a.rollout_versus_greedy(team, act, K, auto_reset=interval)
        frag = b.step_fragment_frames(team, act, auto_reset=interval * K)
        torch.cuda.synchronize()
        for key in KEYS:
            assert _same(a.fragment[key], frag[key]), (it, key, float((a.fragment[key].double() - frag[key].double()).abs().max()))
        assert torch.equal(a.fragment_restarted, frag['restarted'] != 0), it
        assert torch.equal(b.fragment_restarted, frag['restarted'] != 0), it
        assert _same(a.fragment['final_obs'], frag['final_obs']), it
        frames = frag['frames']
        seen_idle |= bool((frames == 0).any())
        seen_early |= bool(((frames > 0) & (frames < K)).any())
        seen_restart |= bool(frag['restarted'].any())
    assert seen_restart and (seen_early or K == 1)
    assert seen_idle or interval == 1 or (K == 1 and not must_idle)


@pytest.mark.parametrize('interval', [1, 2])
@pytest.mark.parametrize('K', [1, 3, 10])
@pytest.mark.parametrize('config', list(CASES))
def test_greedy_opponents_equal_the_fused_fragment(config, K, interval):
    _against_fused(config, K, interval, max_episode_steps=7)


@pytest.mark.parametrize('config', list(CASES))
def test_seven_frame_episodes_leave_fragments_without_a_frame(config):
    """K = 1 under an interval of 2 fragments, seven-frame episodes: every other episode ends on the interval's first call, so the second finds frames = 0."""
    _against_fused(config, 1, 2, max_episode_steps=6, must_idle=True)


# ------------------------------------------------------------------ 3., 4. other opponents, every term: a twin stepped per frame, reduced in NumPy
def _heuristic_targets(e):
    e.set_target_opponent('heuristic')


def _heuristic_cameras(e):
    e.set_camera_opponent('heuristic')


def _mixture(e):
    e.set_opponent_mixture('target', {'naive': 1.0, 'random': 1.0})


def _channel(e):
    e.set_channel('target', dropout_rate=0.3)


OPPONENTS = {'heuristic targets': ('camera', _heuristic_targets), 'heuristic cameras': ('target', _heuristic_cameras),
             'naive:1,random:1 targets': ('camera', _mixture), 'greedy targets, dropout 0.3': ('camera', _channel)}
TERMS = {'camera': ({'raw_reward': 0.5, 'soft_coverage_score': 1.0, 'num_tracked': 0.25}, 'mean'),
         'target': ({'raw_reward': 1.0, 'normalized_goal_distance': -0.5, 'sparse_delivery': 2.0, 'soft_coverage_score': 0.25, 'is_colliding': -1.0, 'is_tracked': -0.5}, 'none')}


def _twin_run(a, b, greedy, team, K, interval, row_dtype, fragments, seed=5, zero_action=False):
    """`a`: per-frame fragments attached; `b`: the twin (same seed, same opponents, transform and overwrite-mode reward rows), stepped per frame
    and reduced by frame_fragment_ref; `greedy`: a third engine with Greedy opponents and no channel (or None), for the vacuity check.
    Returns (the opponents' actions differed from the Greedy engine's somewhere, the twin's term rows seen non-zero [terms])."""
    N = a.num_envs
    agents = a.num_cameras if team == 'camera' else a.num_targets
    D = a.camera_obs_dim if team == 'camera' else a.target_obs_dim
    np_obs = np.float64 if a.obs_dtype == torch.float64 else np.float32
    np_row = np.float64 if row_dtype == torch.float64 else np.float32
    st = R.new_state(N, agents, D, obs_dtype=np_obs, row_dtype=np_row)
    gen = torch.Generator(device='cpu').manual_seed(seed)
    other = 1 if team == 'camera' else 0
    differs, calls, seen = False, 0, None
    for it in range(fragments):
        act = _actions(gen, N, agents, team, a.device)
        if zero_action:
            act.zero_()
        frag = a.step_fragment_frames(team, act, auto_reset=interval * K)
        lost = np.zeros(N, dtype=bool)
        for f in range(K):
            b.step_versus_greedy(team, act, auto_reset=interval * K)
            if greedy is not None:
                greedy.step_versus_greedy(team, act, auto_reset=interval * K)
                differs |= not torch.equal(b.policy_actions()[other], greedy.policy_actions()[other])
            calls += 1
            torch.cuda.synchronize()
            s = b.scalars.cpu().numpy()
            rows = (b.camera_obs if team == 'camera' else b.target_obs).cpu().numpy()
            reward = (b.camera_reward_rows if team == 'camera' else b.target_reward_rows).cpu().numpy()
            terms = (b.camera_reward_terms if team == 'camera' else b.target_reward_terms)
            if terms is not None:
                nz = (terms != 0).reshape(-1, terms.shape[-1]).any(dim=0).cpu().numpy()
                seen = nz if seen is None else seen | nz
            R.fold_frame(st, s, rows, f, K, reward_rows=reward)
            if calls % (interval * K) == 0:
                lost = s[:, 2] == 1                                   # (ended on the closing frame: the twin holds the first row already)
                R.first_rows(st, s, rows)
        torch.cuda.synchronize()
        for key in KEYS + ('restarted',):
            got = frag[key].cpu().numpy()
            assert got.dtype == st[key].dtype and np.array_equal(got, st[key]), (it, key)
        got = frag['final_obs'].cpu().numpy()
        assert np.array_equal(got[~lost], st['final_obs'][~lost]), it
        st['final_obs'][lost] = got[lost]
    return differs, seen


def _build(config, N, seed, obs_dtype, setup, max_episode_steps=7, **kwargs):
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    e = Engine(read_config(config, max_episode_steps=max_episode_steps), N, seed=seed, obs_dtype=obs_dtype, **kwargs)
    e.enable_policies()
    if setup is not None:
        setup(e)
    e.reset()
    return e


def _plant_news(eng):
    """Greedy targets talk about emptied warehouses only, and no random trajectory empties one: warehouses 1 and 2 hold nothing, NO target knows it, every
    other target carries nothing, and all of them stand inside the four warehouses in turn (tests/test_gpu_scripted.py plants the same scene with the
    news already known).  Whoever stands in an empty warehouse learns it on the first frame and tells the others: a lost message then changes a goal."""
    from scripted_ref import WAREHOUSES
    sd = eng.state_dict()
    f = {k: np.array(sd[k], dtype=np.float64, copy=True) for k in ('tgt_x', 'tgt_y', 'tgt_goals', 'tgt_goal_bits', 'freights', 'bounties',
                                                                    'remaining_cargoes', 'awaiting_cargo_counts')}
    rng = np.random.RandomState(3)
    for e in range(eng.num_envs):
        f['remaining_cargoes'][e, 1:3] = 0
        for key in ('tgt_goals', 'tgt_goal_bits', 'freights', 'bounties'):
            f[key][e, ::2] = -1 if key == 'tgt_goals' else 0
        for t in range(eng.num_targets):
            w = (t + e) % 4
            f['tgt_x'][e, t] = WAREHOUSES[w, 0] + rng.uniform(-30.0, 30.0)
            f['tgt_y'][e, t] = WAREHOUSES[w, 1] + rng.uniform(-30.0, 30.0)
        f['awaiting_cargo_counts'][e] = f['remaining_cargoes'][e].sum(axis=0) + f['tgt_goal_bits'][e].sum(axis=0)
    eng.load_state_dict(f)
    eng.observe()


@pytest.mark.parametrize('case', list(OPPONENTS))
def test_other_opponents_equal_the_per_frame_twin(case):
    team, setup = OPPONENTS[case]
    K, interval, N = 3, 2, N_TILES
    shaping = ({'raw_reward': 1.0, 'coverage_rate': 0.5, ('num_tracked' if team == 'camera' else 'is_tracked'): 0.25}, 'none')
    # (a dropped message changes what a Greedy target does only once the targets have news to share: that case gets longer episodes)
    steps, fragments = (25, 14) if 'dropout' in case else (7, 8)
    a, b = (_build('MATE-4v8-9.yaml', N, 31, torch.float64, setup, max_episode_steps=steps) for _ in range(2))
    greedy = _build('MATE-4v8-9.yaml', N, 31, torch.float64, None, max_episode_steps=steps)
    if 'dropout' in case:
        for e in (a, b, greedy):
            _plant_news(e)
    a.enable_fragment_rows(team, K, shaping=shaping, relative_coordinates=True, rescaled_observation=True, first_rows=True, final_obs=True, per_frame=True)
    for e in (b, greedy):
        e.set_obs_transform(True, True)
        e.enable_reward_rows(**{team: shaping})
    differs, _ = _twin_run(a, b, greedy, team, K, interval, torch.float64, fragments=fragments)
    assert differs, 'the opponents acted like the Greedy ones throughout: the case shows nothing'
    if 'dropout' in case:
        sent, delivered = (x.cpu().numpy() for x in b.channel_edges('target'))
        print('messages of the last call: sent', int((sent != 0).sum()), 'delivered', int((delivered != 0).sum()))
    assert (a.state_dict()['episode'] >= 1).any()


@pytest.mark.parametrize('row_dtype', [torch.float32, torch.float64])
def test_soft_coverage_for_a_camera_learner(row_dtype):
    K, N = 3, N_TILES
    a, b = (_build('MATE-4v8-9.yaml', N, 13, torch.float32, _heuristic_targets) for _ in range(2))
    a.enable_fragment_rows('camera', K, shaping=TERMS['camera'], dtype=row_dtype, first_rows=True, final_obs=True, per_frame=True)
    b.enable_reward_rows(camera=TERMS['camera'], dtype=row_dtype, terms=True)
    _, seen = _twin_run(a, b, None, 'camera', K, 1, row_dtype, fragments=6)
    print('camera terms seen non-zero:', seen)
    assert seen[4], 'soft_coverage_score stayed 0'


@pytest.mark.parametrize('row_dtype', [torch.float32, torch.float64])
def test_the_target_terms_on_planted_deliveries(row_dtype):
    """normalized_goal_distance, sparse_delivery, soft_coverage_score and is_colliding for a target learner.  No random policy delivers within an
    episode, so the batch is the planted warehouse scenes of tests/logistics_scenes.py (their own batch size), every probe's target standing inside its
    warehouse: the deliveries happen on the first frame whoever acts."""
    import logistics_scenes as LS
    from test_gpu_info_rows import _flat_of, _planted, _standing
    K = 3
    engines = []
    for _ in range(2):
        eng, scene, flat0 = _planted('MATE-4v8-9')
        eng.import_state(_flat_of(eng, flat0, _standing(scene)))
        eng.observe()
        engines.append(eng)
    a, b = engines
    a.enable_fragment_rows('target', K, shaping=TERMS['target'], dtype=row_dtype, first_rows=True, final_obs=True, per_frame=True)
    b.enable_reward_rows(target=TERMS['target'], dtype=row_dtype, terms=True)
    assert a.num_envs == LS.BATCH
    _, seen = _twin_run(a, b, None, 'target', K, 1, row_dtype, fragments=6, seed=11)
    print('target terms seen non-zero:', seen)
    for k, key in ((4, 'normalized_goal_distance'), (5, 'sparse_delivery'), (6, 'soft_coverage_score'), (8, 'is_colliding')):
        assert seen[k], key + ' stayed 0'
    assert bool((a.fragment['shaped'] != 0).any())


# ------------------------------------------------------------------ 5. graph replay
def test_graph_replay_equals_direct_calls():
    K, N = 5, N_TILES
    shaping = ({'coverage_rate': 1.0, 'soft_coverage_score': 0.5}, 'mean')
    engines = [_build('MATE-4v8-9.yaml', N, 9, torch.float32, _heuristic_targets) for _ in range(2)]
    for e in engines:
        e.enable_fragment_rows('camera', K, shaping=shaping, relative_coordinates=True, rescaled_observation=True, first_rows=True, final_obs=True, per_frame=True)
    a, b = engines                                         # graph-replayed | launched directly
    act = torch.zeros((N, a.num_cameras, 2), dtype=torch.float64, device=a.device)
    stepper = a.make_stepper(act, None, auto_reset=2 * K, graph_steps=2, versus='camera', frame_skip=K)
    assert stepper.per_frame and stepper.fragment['obs'] is a.fragment_obs
    for _ in range(stepper.warmup_steps):
        b.step_fragment_frames('camera', act, auto_reset=2 * K)
    gen = torch.Generator(device='cpu').manual_seed(2)
    restarted = False
    for replay in range(4):
        act.copy_(_actions(gen, N, a.num_cameras, 'camera', a.device))
        if replay == 2:                                    # a schedule: rewritten in place between two replays
            for e in (a, b):
                e.fragment['coefficients'][1] = 3.0
        stepper.run(2)
        for _ in range(2):
            b.step_fragment_frames('camera', act, auto_reset=2 * K)
        torch.cuda.synchronize()
        for key in KEYS + ('restarted', 'final_obs'):
            assert _same(a.fragment[key], b.fragment[key]), (replay, key)
        restarted |= bool(a.fragment['restarted'].any())
    assert restarted
    stepper.close()


# ------------------------------------------------------------------ 6. inertness
def test_attached_engine_steps_like_an_unattached_twin():
    K, N = 3, N_TILES
    a, b = (_build('MATE-4v8-9.yaml', N, 21, torch.float32, _heuristic_targets) for _ in range(2))
    a.enable_fragment_rows('camera', K, first_rows=True, final_obs=True, per_frame=True)
    gen = torch.Generator(device='cpu').manual_seed(8)
    for it in range(4 * K):
        act = _actions(gen, N, a.num_cameras, 'camera', a.device)
        for e in (a, b):
            e.step_versus_greedy('camera', act, auto_reset=K)
        torch.cuda.synchronize()
        for name in ('camera_obs', 'target_obs', 'scalars', 'masks'):
            assert torch.equal(getattr(a, name), getattr(b, name)), (it, name)
    assert torch.equal(a.export_state(), b.export_state())


def test_the_records_keep_the_parents_kernels():
    lib, golden = os.path.join(ROOT, 'mate_amd', 'lib'), os.path.join(ROOT, 'tests', 'golden', 'frame_fragment_parent_records')
    names = sorted(os.listdir(golden))
    assert 'kernel_resources_opponents.json' in names and len(names) == 8
    for name in names:
        with open(os.path.join(lib, name), 'rb') as x, open(os.path.join(golden, name), 'rb') as y:
            built, parent = x.read(), y.read()
        if name != 'kernel_resources_opponents.json':
            assert built == parent, name
            continue
        built, parent = json.loads(built), json.loads(parent)
        assert {k: built[k] for k in parent} == parent
        new = {k: r for k, r in built.items() if k not in parent}
        assert len(new) == 2 and all('fragment_frame_kernel' in k for k in new)
        for r in new.values():
            assert r['VGPRs'] <= 128 and r['Occupancy'] >= 4 and r['SGPRs Spill'] == 0 and r['VGPRs Spill'] == 0 and r['ScratchSize'] == 0 and r['Dynamic Stack'] == 'False'


# ------------------------------------------------------------------ 7. the stack
def test_the_stack_of_attachments_against_each_alone():
    K, N = 3, N_TILES

    def run(state, info, episodes, frames):
        e = _build('MATE-4v8-9.yaml', N, 17, torch.float32, _heuristic_targets)
        if frames:
            e.enable_fragment_rows('camera', K, shaping=TERMS['camera'], first_rows=True, final_obs=True, per_frame=True)
        else:
            e.enable_reward_rows(camera=TERMS['camera'])
        if state:
            e.enable_state_rows()
        if info:
            e.enable_info_rows()
        if episodes:
            e.enable_episode_records('camera')
        gen = torch.Generator(device='cpu').manual_seed(4)
        for _ in range(5):
            act = _actions(gen, N, e.num_cameras, 'camera', e.device)
            for _ in range(K):
                e.step_versus_greedy('camera', act, auto_reset=K)
        torch.cuda.synchronize()
        out = {}
        if frames:
            out.update({'fragment ' + k: e.fragment[k].clone() for k in KEYS + ('restarted', 'final_obs')})
        if state:
            out['state'] = e.state.clone()
        if info:
            out.update({'info ' + k: v.clone() for k, v in e.info().items()})
        if episodes:
            records = e.episode_records()[0]                  # (the ring's order is the order of arrival: sorted by environment, then episode)
            out['episodes'] = records[torch.argsort(records[:, 0] * 4096 + records[:, 1])].clone()
        return out

    everything = run(True, True, True, True)
    assert any(k.startswith('fragment') for k in everything) and 'state' in everything and 'episodes' in everything
    for alone in ((True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True)):
        for key, value in run(*alone).items():
            assert torch.equal(everything[key], value) or (value.is_floating_point() and torch.equal(torch.nan_to_num(everything[key], nan=-7.0), torch.nan_to_num(value, nan=-7.0))), (alone, key)


# ------------------------------------------------------------------ 8. refusals and facades
def test_refusals_and_detach():
    from mate_amd._native import EngineError, MateFrameFragments, MateStepIO
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    N, K = 8, 3
    eng = Engine(read_config('MATE-4v2-9.yaml'), N, seed=1)
    eng.enable_policies()
    lib, err = eng.lib, lambda: eng.lib.mate_engine_last_error().decode()  # noqa: E731
    buf = torch.zeros(N * 64, dtype=torch.float64, device=eng.device)
    ok = MateFrameFragments()
    ok.team, ok.frames, ok.out_dtype, ok.frames_dev = 0, K, 1, buf.data_ptr()
    assert lib.mate_engine_enable_frame_fragments(eng._h, ctypes.byref(ok)) == -4 and 'before reset' in err()       # MATE_ESTATE
    eng.reset()

    def refused(code, word, **fields):
        cfg = MateFrameFragments()
        cfg.team, cfg.frames, cfg.out_dtype, cfg.frames_dev = 0, K, 1, buf.data_ptr()
        for k, v in fields.items():
            setattr(cfg, k, v)
        assert lib.mate_engine_enable_frame_fragments(eng._h, ctypes.byref(cfg)) == code and word in err(), (fields, err())
        assert eng.lib.mate_engine_frame_fragment(eng._h, ctypes.byref(cfg), ctypes.byref(MateStepIO()), 0, 0, None) != 0

    refused(-1, 'team', team=2)
    refused(-1, 'frames', frames=0)
    refused(-1, 'out_dtype', out_dtype=7)
    refused(-1, 'aligned', rewards_dev=buf.data_ptr() + 4)
    refused(-1, 'aligned', obs_dev=buf.data_ptr() + 2)
    refused(-1, 'frames_dev', info_dev=buf.data_ptr(), frames_dev=None)
    refused(-1, 'first_rows', first_rows=1)
    refused(-4, 'overwrite mode', shaped_dev=buf.data_ptr())                    # no reward rows attached
    eng.enable_reward_rows(camera=({'raw_reward': 1.0}, 'none'), accumulate=True)
    refused(-4, 'overwrite mode', shaped_dev=buf.data_ptr())                    # accumulating ones
    eng.enable_reward_rows(camera=({'raw_reward': 1.0}, 'none'), dtype=torch.float32)
    refused(-1, 'out_dtype', shaped_dev=buf.data_ptr())                         # of another type
    eng.disable_reward_rows()
    nav = Engine(read_config('MATE-Navigation.yaml'), N, seed=1)
    nav.reset()
    with pytest.raises(EngineError, match='no cameras') as info:
        nav.enable_fragment_rows('camera', K, per_frame=True)
    assert info.value.code == -1
    assert eng.fragment is None

    act = torch.zeros((N, eng.num_cameras, 2), dtype=torch.float64, device=eng.device)
    eng.step_versus_greedy('camera', act, auto_reset=2 * K)                     # opens an interval
    with pytest.raises(EngineError, match='open restart interval') as info:
        eng.enable_fragment_rows('camera', K, per_frame=True)
    assert info.value.code == -4 and eng.fragment is None
    eng.reset()
    eng.enable_fragment_rows('camera', K, per_frame=True)
    frames = eng.fragment_frames
    for bad in (True, 0, K + 1, 2):
        with pytest.raises(EngineError, match='multiple') as info:
            eng.step_versus_greedy('camera', act, auto_reset=bad)
        assert info.value.code == -1
    io = MateStepIO()
    io.camera_actions_dev = act.data_ptr()
    io.act_dtype = 1
    assert lib.mate_engine_step_versus_greedy(eng._h, 0, ctypes.byref(io), None, K, None) == -1 and 'scalars_dev' in err()
    torch.cuda.synchronize()
    assert int(frames.max()) == 0                                                # a refused call changed nothing
    with pytest.raises(EngineError, match='pipelined') as info:
        eng.rollout_greedy(2, auto_reset='pipelined')
    assert info.value.code == -4
    # the other team's calls and the other flows do not enqueue it
    frames.fill_(-1)
    tgt_act = torch.zeros((N, eng.num_targets, 2), dtype=torch.float64, device=eng.device)
    eng.step_versus_greedy('target', tgt_act, auto_reset=K)
    eng.step_greedy(auto_reset=K)
    eng.step_random(auto_reset=K)
    torch.cuda.synchronize()
    assert int(frames.max()) == -1
    eng.reset()
    eng.step_fragment_frames('camera', act)
    torch.cuda.synchronize()
    assert int(frames.min()) == K
    eng.disable_fragment_rows()
    assert eng.fragment is None and eng.fragment_obs is None
    frames.fill_(-1)
    eng.step_versus_greedy('camera', act, auto_reset=True)                       # detached: any auto_reset again
    torch.cuda.synchronize()
    assert int(frames.max()) == -1


def test_two_groups_are_one_engine():
    from mate_amd.config import read_config
    from mate_amd.engine import Engine, EngineGroups
    cfg = read_config('MATE-4v8-9.yaml', max_episode_steps=7)
    K, N = 3, 32
    whole = Engine(cfg, N, seed=6)
    groups = EngineGroups(cfg, N, groups=2, seed=6, policies=True)
    whole.enable_policies()
    whole.set_target_opponent('heuristic')
    groups.each(lambda g, e: e.set_target_opponent('heuristic'))
    whole.reset()
    groups.reset()
    whole.enable_fragment_rows('camera', K, first_rows=True, per_frame=True)
    groups.enable_fragment_rows('camera', K, first_rows=True, per_frame=True)
    gen = torch.Generator(device='cpu').manual_seed(3)
    for _ in range(5):
        act = _actions(gen, N, whole.num_cameras, 'camera', whole.device)
        whole.step_fragment_frames('camera', act)
        frags = groups.step_fragment_frames('camera', [act[:16].contiguous(), act[16:].contiguous()])
        groups.synchronize()
        torch.cuda.synchronize()
        for key in ('obs', 'rewards', 'done', 'frames', 'info', 'restarted'):
            assert torch.equal(whole.fragment[key], torch.cat([f[key] for f in frags])), key


@pytest.mark.parametrize('case', ['heuristic targets', 'the target terms'])
def test_batched_environment_per_frame(case):
    from mate_amd.environment import BatchedMultiAgentTracking
    K, N = 3, N_TILES
    if case == 'heuristic targets':
        kwargs = dict(learner='camera', target_agent='heuristic', camera_reward_shaping=TERMS['camera'])
    else:
        kwargs = dict(learner='target', camera_agent='heuristic', target_reward_shaping=TERMS['target'])
    env = BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=N, seed=4, obs_dtype=torch.float64, relative_coordinates=True, rescaled_observation=True,
                                    frame_skip=K, per_frame=True, first_rows=True, max_episode_steps=7, **kwargs)
    team = kwargs['learner']
    ref = BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=N, seed=4, obs_dtype=torch.float64, relative_coordinates=True, rescaled_observation=True,
                                    max_episode_steps=7, **{k: v for k, v in kwargs.items() if k.endswith('_agent')})
    obs = env.reset()
    first = ref.reset()[0 if team == 'camera' else 1]
    agents = env.num_cameras if team == 'camera' else env.num_targets
    assert obs.shape == first.shape and torch.equal(obs, first)                  # the packer's transformed rows of reset()
    gen = torch.Generator(device='cpu').manual_seed(1)
    total = 0
    for _ in range(4):
        act = _actions(gen, N, agents, team, env.device)
        obs, rewards, done, info = env.step_fragment(act)
        torch.cuda.synchronize()
        assert rewards.shape == (N, agents) and rewards is env.engine.fragment_shaped
        assert set(info) == {'raw_reward', 'normalized_raw_reward', 'coverage_rate', 'real_coverage_rate', 'mean_transport_rate', 'num_delivered_cargoes', 'frames',
                             'restarted', 'final_observation'}
        assert torch.equal(info['restarted'], done)                              # auto_reset = 1 fragment: what ended restarted behind it
        total += int(info['frames'].sum())
    assert total == N * 11                                                       # eight-frame episodes: 3 + 3 + 2 (one idle slot), then 3 of the next


@pytest.mark.parametrize('obs_dtype', [torch.float32, torch.float64])
def test_generic_shape_with_a_ragged_row(obs_dtype):
    import shape_edges
    from mate_amd.engine import Engine
    shape = (7, 5, 3)
    N, K = N_TILES, 3                                      # 7v5-3: no compiled specialisation, target rows of 5 x 113 elements
    engines = []
    for _ in range(2):
        e = Engine(shape_edges.scenario(shape), N, seed=3, obs_dtype=obs_dtype)
        assert not e.specialised
        e.enable_policies()
        e.reset()
        engines.append(e)
    a, b = engines
    A, D = a.num_targets, a.target_obs_dim
    assert (A * D * (4 if obs_dtype == torch.float32 else 8)) % 16 != 0
    a.enable_fragment_rows('target', K, first_rows=True, final_obs=True, per_frame=True)
    b.enable_reward_rows(target=({'raw_reward': 1.0}, 'none'))
    a.fragment_obs.fill_(12345.0)
    st_rows = None
    act = torch.zeros((N, A, 2), dtype=torch.float64, device=a.device)
    frag = a.step_fragment_frames('target', act)
    for f in range(K):
        b.step_versus_greedy('target', act, auto_reset=K)
        if f == K - 1:
            st_rows = b.target_obs.clone()
    torch.cuda.synchronize()
    assert int(frag['frames'].min()) == K and not bool(frag['restarted'].any())
    assert torch.equal(frag['obs'], st_rows)
