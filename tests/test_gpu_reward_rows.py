"""GPU (-m gpu): the shaped reward rows (Engine.enable_reward_rows: the reference's AuxiliaryCameraRewards / AuxiliaryTargetRewards
as one launch attached to the engine) against the traces the reference's wrappers shaped, the example trainers' chains, the torch
shapers on the engine's own draws, a twin engine across the terminal step and the restart, graph replay, and the error returns."""
import ctypes

import numpy as np
import pytest
import torch

import golden_util as G
import gpu_util as U

pytestmark = pytest.mark.gpu

CAMERA_KEYS = ('raw_reward', 'coverage_rate', 'real_coverage_rate', 'mean_transport_rate', 'soft_coverage_score', 'num_tracked', 'baseline')
TARGET_KEYS = ('raw_reward', 'coverage_rate', 'real_coverage_rate', 'mean_transport_rate', 'normalized_goal_distance',
               'sparse_delivery', 'soft_coverage_score', 'is_tracked', 'is_colliding', 'baseline')
RECORD_TERMS = ('raw_reward', 'coverage_rate', 'real_coverage_rate', 'mean_transport_rate')      # from the f32 step record
INTEGER_TERMS = ('sparse_delivery', 'is_tracked', 'is_colliding', 'num_tracked')
MATE_EINVAL, MATE_ESTATE = -1, -4


def _replay(eng, fx, s, N):
    Nc, Nt, dev = eng.num_cameras, eng.num_targets, eng.device
    ca = torch.from_numpy(np.broadcast_to(fx['step/cam_act'][s], (N, Nc, 2)).copy()).to(dev)
    ta = torch.from_numpy(np.broadcast_to(fx['step/tgt_act'][s], (N, Nt, 2)).copy()).to(dev)
    tape = torch.from_numpy(np.broadcast_to(np.nan_to_num(fx['step/tape_ct'][s], nan=0.0), (N, Nc, Nt)).copy()).to(dev)
    goal = torch.from_numpy(np.broadcast_to(np.nan_to_num(fx['step/goal_u'][s], nan=0.0), (N, Nt)).copy()).to(dev)
    return eng.step(ca, ta, tape_ct=tape, tape_goal=goal, auto_reset=False)


def _install_outer_tables(eng, fx, N):
    eng.enable_outer_boundary()
    for c, (phis, rhos) in enumerate(G.luts_of(fx, outer=True)):
        for e in range(N):
            eng.lut_write(e, c, phis, rhos, outer=True)


# ---------------------------------------------------------------------------------------------- 1, 2: the reference's fixtures
@pytest.mark.parametrize('name', ['auxtgt_4v8-9_s11', 'auxtgt_8v8-9_s12', 'auxtgt_4v2-9_s13', 'auxtgt_nav_s14'])
def test_target_rows_on_the_reference_fixtures(name):
    """Rows and terms attached, on the traces the reference's AuxiliaryTargetRewards shaped: every term against step/auxt_<key>
    (per-target terms 1e-9, the four f32-record terms 1e-6, integer-valued terms exact), the shaped reward against
    step/aux_reward_tgt (rtol 1e-6 / atol 1e-5): the bars of test_auxiliary_target_rewards_fixtures."""
    fx = G.load(name + '.npz')
    N = 3
    eng = U.engine_from_fixture(fx, N, obs_dtype=torch.float32)
    keys, coef, reduction = [str(k) for k in fx['auxt_keys']], [float(c) for c in fx['auxt_coefficients']], str(fx['auxt_reduction'])
    if 'soft_coverage_score' in keys:
        _install_outer_tables(eng, fx, N)
    eng.enable_reward_rows(target=(dict(zip(keys, coef)), reduction), terms=True)
    assert eng.camera_reward_rows is None and eng.target_reward_rows.shape == (N, eng.num_targets)
    seen_delivery = False
    for s in range(len(fx['step/done'])):
        _replay(eng, fx, s, N)
        shaped, terms = eng.target_reward_rows.cpu().numpy(), eng.target_reward_terms.cpu().numpy()
        for key in keys:
            term, ref = terms[:, :, TARGET_KEYS.index(key)], fx['step/auxt_' + key][s]
            tol = 1e-6 if key in RECORD_TERMS else 1e-9
            for e in range(N):
                np.testing.assert_allclose(term[e], ref, rtol=tol, atol=tol, err_msg=f'{key} step {s}')
                if key in INTEGER_TERMS:
                    assert np.array_equal(term[e], np.asarray(ref, dtype=np.float64)), (key, s)
        for e in range(N):
            np.testing.assert_allclose(shaped[e], fx['step/aux_reward_tgt'][s], rtol=1e-6, atol=1e-5, err_msg=str(s))
        seen_delivery |= bool(fx['step/auxt_sparse_delivery'][s].any()) if 'sparse_delivery' in keys else False
    assert seen_delivery == (name in ('auxtgt_4v8-9_s11', 'auxtgt_8v8-9_s12'))     # the delivery term is exercised


@pytest.mark.parametrize('name', ['softcov_4v8-9_s8', 'softcov_8v8-9_s9', 'softcov_4v2-9_s10'])
def test_camera_rows_on_the_reference_fixtures(name):
    """... and the camera team on the traces AuxiliaryCameraRewards shaped (reductions none / mean / max): step/aux_reward_cam at
    1e-6 (f32 step record), the soft coverage term at 1e-9, num_tracked exact against the fixture's mask."""
    fx = G.load(name + '.npz')
    N = 3
    eng = U.engine_from_fixture(fx, N, obs_dtype=torch.float32)
    _install_outer_tables(eng, fx, N)
    keys, coef, reduction = [str(k) for k in fx['aux_keys']], [float(c) for c in fx['aux_coefficients']], str(fx['aux_reduction'])
    eng.enable_reward_rows(camera=(dict(zip(keys, coef)), reduction), terms=True)
    for s in range(len(fx['step/done'])):
        _replay(eng, fx, s, N)
        shaped, terms = eng.camera_reward_rows.cpu().numpy(), eng.camera_reward_terms.cpu().numpy()
        tracked = fx['step/camera_target_view_mask'][s].astype(bool).sum(axis=1).astype(np.float64)
        for e in range(N):
            np.testing.assert_allclose(shaped[e], fx['step/aux_reward_cam'][s], rtol=1e-6, atol=1e-6, err_msg=str(s))
            assert np.array_equal(terms[e, :, CAMERA_KEYS.index('num_tracked')], tracked), s
            if 'soft_coverage_score' in keys:
                np.testing.assert_allclose(terms[e, :, CAMERA_KEYS.index('soft_coverage_score')], fx['step/soft_coverage_score'][s],
                                           rtol=1e-9, atol=1e-9, err_msg=str(s))


# ---------------------------------------------------------------------------------------------- 3: the example trainers' chains
@pytest.mark.parametrize('name', ['chain_4v8-9_s15', 'chain_target_2v4-0_s16'])
def test_rows_along_the_example_trainers_chains(name):
    """The chains of tests/test_gpu_chain.py (grid indices, fused transforms, step_versus_greedy on the recorded draws) with the
    rows attached: per frame against step/chain_reward_*, and on a second engine accumulating, zeroed at every learner step,
    against FrameSkip's skip/reward_* -- that file's tolerances."""
    from test_gpu_chain import _tapes
    from mate_amd.environment import BatchedMultiAgentTracking
    fx = G.load(name + '.npz')
    team = str(fx['learner_team'])
    me = 'cam' if team == 'camera' else 'tgt'
    N, levels = 2, int(fx['discrete_levels'])
    keys, coef, reduction = [str(k) for k in fx['aux_keys']], fx['aux_coefficients'], str(fx['aux_reduction'])
    shaping = (dict(zip(keys, (float(c) for c in coef))), reduction)
    engines = []
    for accumulate in (False, True):
        env = BatchedMultiAgentTracking(U.config_of_fixture(fx), num_envs=N, obs_dtype=torch.float32, auto_reset=False, relative_coordinates=True,
                                        rescaled_observation=True, **{f'discrete_{team}_levels': levels})
        eng = U.load_fixture_state(env.engine, fx)
        env.enable_greedy_policies()
        eng.enable_reward_rows(**{team: shaping}, accumulate=accumulate)
        tape0 = torch.from_numpy(np.where(fx['reset/camera_target_view_mask'], 1.0, 0.0)[None].repeat(N, 0)).to(eng.device)
        eng.observe(tape_ct=tape0)
        engines.append(eng)
    per_frame, summed = engines
    rows = (lambda eng: eng.camera_reward_rows) if team == 'camera' else (lambda eng: eng.target_reward_rows)
    learner = fx['step/learner_step']
    for s in range(len(fx['step/done'])):
        if s == 0 or learner[s] != learner[s - 1]:
            if s:
                got = rows(summed).cpu().numpy()
                for e in range(N):
                    np.testing.assert_allclose(got[e], fx[f'skip/reward_{me}'][learner[s - 1]], rtol=1e-6, atol=5e-6 if team == 'camera' else 1e-4)
            rows(summed).zero_()
        for eng in engines:
            policy, tape_ct, tape_goal, idx = _tapes(fx, s, N, eng.device, team)
            eng.step_versus_greedy(team, idx, policy_tape=policy, tape_ct=tape_ct, tape_goal=tape_goal, auto_reset=False)
        got = rows(per_frame).cpu().numpy()
        for e in range(N):
            if team == 'camera':
                np.testing.assert_allclose(got[e], fx['step/chain_reward_cam'][s], rtol=0, atol=1e-6, err_msg=str(s))
            else:
                np.testing.assert_allclose(got[e], fx['step/chain_reward_tgt'][s], rtol=1e-6, atol=1e-5, err_msg=str(s))
    got = rows(summed).cpu().numpy()
    np.testing.assert_allclose(got[0], fx[f'skip/reward_{me}'][learner[-1]], rtol=1e-6, atol=5e-6 if team == 'camera' else 1e-4)


# ---------------------------------------------------------------------------------------------- 4: the torch shapers, own draws
CAMERA_COEFFICIENTS = dict(zip(CAMERA_KEYS, (1.0, 0.5, -0.25, 2.0, 0.125, 0.75, -1.0)))
TARGET_COEFFICIENTS = dict(zip(TARGET_KEYS, (1.0, -0.5, 0.25, 2.0, -3.0, 10.0, 0.125, -0.75, -1.5, 0.5)))
REDUCTION_PAIRS = [('none', 'none'), ('mean', 'mean'), ('sum', 'sum'), ('max', 'max'), ('min', 'none')]


def _sixteen_by_sixteen():
    from mate_amd.config import read_config
    cfg = read_config('MATE-8v8-9.yaml')
    cfg['name'] = 'MultiAgentTracking(16v16, 9)'
    cam = cfg['camera']['location_random_range']
    more = [[-x1, -x0, y0, y1] if i % 2 else [x0, x1, -y1, -y0] for i, (x0, x1, y0, y1) in enumerate(cam)]
    cfg['camera']['location_random_range'] = [[float(v) for v in box] for box in cam + more]
    cfg['target']['location_random_range'] = [[-300.0, 300.0, -300.0, 300.0]] * 16
    return cfg


def _few_cargo_engine(n, seed):
    """MATE-4v8-9 with only the cargoes in transit left, as the obsmode_4v8-9_fewcargo fixture's scenario is built (make_golden.py
    tweak_few_cargoes); two targets are put where such an episode ends up -- unloaded, one knowing three warehouses empty, one all
    four -- so that both "no goal" branches are inputs of the first step already."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    eng = Engine(read_config('MATE-4v8-9.yaml'), n, seed=seed)
    eng.enable_policies()
    eng.reset()
    sd = eng.state_dict()
    goals, bits, empty = sd['tgt_goals'].copy(), sd['tgt_goal_bits'].copy(), sd['tgt_empty_bits'].copy()
    goals[:, :2], bits[:, :2] = -1, 0
    empty[:, 0], empty[:, 1] = [1, 1, 1, 0], [1, 1, 1, 1]
    awaiting = np.zeros_like(sd['awaiting_cargo_counts'])
    for e in range(n):
        for t in range(eng.num_targets):
            if goals[e, t] >= 0:
                awaiting[e, int(goals[e, t])] += bits[e, t, int(goals[e, t])]
    eng.load_state_dict({'remaining_cargoes': np.zeros_like(sd['remaining_cargoes']), 'awaiting_cargo_counts': awaiting,
                         'tgt_goals': goals, 'tgt_goal_bits': bits, 'tgt_empty_bits': empty})
    return eng


def _builtin_engine(config, n, seed):
    from mate_amd.engine import Engine
    eng = Engine(config, n, seed=seed)
    eng.enable_policies()
    eng.reset()
    return eng


def camera_shaper(eng, coefficients, reduction, view):
    """(terms {key: [N, Nc]}, rows [N, Nc]) f64: the camera shaper's arithmetic (BatchedMultiAgentTracking.auxiliary_camera_rewards) on the step
    Engine.scalars describes, `view` its unpacked camera_target_view_mask; the soft coverage score only where a coefficient names it."""
    N, Nc, dev = eng.num_envs, eng.num_cameras, eng.device
    sc = eng.scalars.double()
    seen = torch.from_numpy(np.asarray(view)).to(dev)
    terms = {'raw_reward': sc[:, 0:1].expand(N, Nc), 'coverage_rate': sc[:, 3:4].expand(N, Nc), 'real_coverage_rate': sc[:, 4:5].expand(N, Nc),
             'mean_transport_rate': sc[:, 5:6].expand(N, Nc),
             'num_tracked': seen.sum(dim=2).double(), 'baseline': torch.ones((N, Nc), dtype=torch.float64, device=dev)}
    if 'soft_coverage_score' in coefficients:
        terms['soft_coverage_score'] = eng.soft_coverage()[1]
    rows = torch.zeros((N, Nc), dtype=torch.float64, device=dev)
    for key, c in coefficients.items():
        rows = rows + c * terms[key]
    if reduction != 'none':
        one = {'mean': rows.mean(dim=1), 'sum': rows.sum(dim=1), 'max': rows.max(dim=1).values, 'min': rows.min(dim=1).values}[reduction]
        rows = one[:, None].expand(N, Nc)
    return terms, rows


SHAPER_BAR = 1e-9                                # rows and terms against the torch shapers on the same records (tests/stack_cases.py imports it)
STRADDLING = ('7v5-3', '16v15-3', '5v7-0')        # tests/shape_edges.py ATTACHED_CASES: camera_target_view_mask rows that cross a 32-bit word


@pytest.mark.parametrize('scenario', ['MATE-8v8-9 x 65', '16v16 x 5', 'few cargoes'] + list(STRADDLING) + ['0v5-64'])
def test_rows_equal_the_torch_shapers_on_the_engines_own_draws(scenario):
    """Both teams, every term and all reductions under step_greedy (auto_reset = 0) against the torch shapers
    (BatchedMultiAgentTracking.auxiliary_camera_rewards' arithmetic, mate_amd.auxiliary_rewards.AuxiliaryTargetRewards) on the same
    records: integer-valued terms exact, everything else 1e-9 (sixteen f64 additions of magnitudes <= 1e3 stay below 1e-10 whatever the
    order).  65 environments: not a multiple of the sixteen per workgroup; 16 x 16: the mask bits span eight words, every row on a
    half-word.  7v5-3, 16v15-3, 5v7-0: rows that cross a word at odd bit positions (this kernel reads them bit by bit through view_bit, not
    through view_row), the frames with seen targets on both sides counted from the unpacked masks the references read; 0v5-64: no cameras, the target rows alone (the camera team is refused: tests/test_gpu_attached_edges.py)."""
    import shape_edges
    from mate_amd.auxiliary_rewards import AuxiliaryTargetRewards
    from mate_amd.config import read_config
    from mate_amd import constants as consts
    target_coefficients = TARGET_COEFFICIENTS
    if scenario == 'MATE-8v8-9 x 65':
        eng = _builtin_engine(read_config('MATE-8v8-9.yaml'), 65, seed=17)
    elif scenario == '16v16 x 5':
        eng = _builtin_engine(_sixteen_by_sixteen(), 5, seed=18)
        assert not eng.specialised and eng.num_cameras * eng.num_targets == 256
    elif scenario == 'few cargoes':
        eng = _few_cargo_engine(6, seed=19)
    else:
        from mate_amd.engine import Engine
        case = shape_edges.attached_case(scenario)
        eng = Engine(shape_edges.case_scenario(case), case.n, seed=case.seed, first_env_index=case.first)
        eng.enable_policies()
        eng.reset()
        assert not eng.specialised and (eng.num_cameras, eng.num_targets, eng.num_obstacles) == case.shape
        if not eng.num_cameras:      # (the soft coverage score takes a maximum over the cameras)
            target_coefficients = {key: c for key, c in TARGET_COEFFICIENTS.items() if key != 'soft_coverage_score'}
    N, Nc, Nt, dev = eng.num_envs, eng.num_cameras, eng.num_targets, eng.device
    branches = {'nearest non-empty': 0, 'all empty': 0}
    straddling = {c: 0 for c in shape_edges.straddling_rows(Nc, Nt)}
    assert bool(straddling) == (scenario in STRADDLING)
    for cam_reduction, tgt_reduction in REDUCTION_PAIRS:
        eng.enable_reward_rows(camera=(CAMERA_COEFFICIENTS, cam_reduction) if Nc else None, target=(target_coefficients, tgt_reduction), terms=True)
        shaper = AuxiliaryTargetRewards(eng, target_coefficients, tgt_reduction)
        for s in range(4):
            eng.step_greedy(auto_reset=0)
            ref_t = shaper()
            for c, frames in shape_edges.straddling_frames(eng.unpack_masks()['camera_target_view_mask']).items():
                straddling[c] += frames
            for k, key in enumerate(TARGET_KEYS):
                if key not in target_coefficients:
                    continue
                got, ref = eng.target_reward_terms[:, :, k], shaper.terms[key]
                assert float((got - ref).abs().max()) <= SHAPER_BAR, (scenario, tgt_reduction, s, key)
                if key in INTEGER_TERMS:
                    assert torch.equal(got, ref.contiguous()), (scenario, s, key)
            assert float((eng.target_reward_rows - ref_t).abs().max()) <= SHAPER_BAR, (scenario, tgt_reduction, s)
            if not Nc:
                assert eng.camera_reward_rows is None and float(eng.target_reward_terms[:, :, TARGET_KEYS.index('is_tracked')].abs().sum()) == 0.0
                continue
            # the camera shaper's arithmetic (environment.py auxiliary_camera_rewards) on the same records
            terms, ref_c = camera_shaper(eng, CAMERA_COEFFICIENTS, cam_reduction, eng.unpack_masks()['camera_target_view_mask'])
            for k, key in enumerate(CAMERA_KEYS):
                assert float((eng.camera_reward_terms[:, :, k] - terms[key]).abs().max()) <= SHAPER_BAR, (scenario, s, key)
            assert torch.equal(eng.camera_reward_terms[:, :, 5], terms['num_tracked'].contiguous())
            assert float((eng.camera_reward_rows - ref_c).abs().max()) <= SHAPER_BAR, (scenario, cam_reduction, s)
            # which goal-distance branches the inputs reached (the torch shaper's own inputs: the exported state)
            sd = eng.state_dict()
            no_goal, known_empty = sd['tgt_goals'] < 0, sd['tgt_empty_bits'].astype(bool).all(axis=2)
            branches['nearest non-empty'] += int((no_goal & ~known_empty).sum())
            branches['all empty'] += int((no_goal & known_empty).sum())
            if no_goal.any():
                assert float(shaper.terms['normalized_goal_distance'][torch.from_numpy(no_goal & known_empty).to(dev)].sub(0.5).abs().sum()) == 0.0
    assert consts.TERRAIN_WIDTH == 2000.0
    if scenario == 'few cargoes':
        assert branches['nearest non-empty'] > 0 and branches['all empty'] > 0, branches
    if straddling:      # the rows the references read did have seen targets on both sides of their word boundary
        print(scenario, 'step_greedy: frames per straddling row', straddling)
        assert min(straddling.values()) >= 1, straddling


# ---------------------------------------------------------------------------------------------- 5: terminal step and restart
def _short_episodes(n, seed, max_episode_steps=6):
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    eng = Engine(read_config('MATE-4v2-9.yaml', max_episode_steps=max_episode_steps), n, seed=seed)
    eng.reset()
    return eng


def test_terminal_step_and_restart_against_a_twin():
    """auto_reset = 1: at the `done` step the rows are those of a twin stepped with auto_reset = 0, bit for bit (the launch runs ahead
    of the restart; the torch shaper reads the restarted records), and the snapshot behind the restart holds the new episode's goals:
    the next step's terms equal the twin's after an explicit masked reset."""
    shaping = dict(camera=({'raw_reward': 1.0, 'num_tracked': 0.5}, 'mean'), target=(dict(TARGET_COEFFICIENTS, soft_coverage_score=0.0), 'none'), terms=True)
    a, b = _short_episodes(40, 23), _short_episodes(40, 23)
    for eng in (a, b):
        eng.enable_reward_rows(**{k: v for k, v in shaping.items()})
    finished = 0
    for s in range(14):
        a.step_random(auto_reset=1, want_masks=True)
        b.step_random(auto_reset=0, want_masks=True)
        assert torch.equal(a.scalars, b.scalars), s
        for name in ('camera_reward_rows', 'target_reward_rows', 'camera_reward_terms', 'target_reward_terms'):
            assert torch.equal(getattr(a, name), getattr(b, name)), (s, name)
        done = b.scalars[:, 2] > 0
        if bool(done.any()):
            finished += int(done.sum())
            assert not torch.equal(a.export_state(), b.export_state())      # `a` has restarted: its records are the new episode's
            b.reset(env_mask=done)
            assert torch.equal(a.export_state(), b.export_state()), s
    assert finished >= 80         # every environment ended (the time limit) twice


def test_idling_environments_contribute_nothing():
    """auto_reset = 4: an environment that waits for the batched restart (done == 2 in its scalar record) has zero rows, and adds
    nothing to accumulating ones."""
    shaping = dict(camera=({'baseline': 1.0, 'num_tracked': 1.0}, 'none'), target=({'baseline': 2.0, 'normalized_goal_distance': 1.0}, 'sum'))
    a, b = _short_episodes(24, 29), _short_episodes(24, 29)
    a.enable_reward_rows(**shaping, terms=True)
    b.enable_reward_rows(**shaping, accumulate=True)
    idled = 0
    for s in range(9):
        b.camera_reward_rows.zero_(), b.target_reward_rows.zero_()
        a.step_random(auto_reset=4, want_masks=True)
        b.step_random(auto_reset=4, want_masks=True)
        idle = a.scalars[:, 2] == 2
        idled += int(idle.sum())
        for eng in (a, b):
            assert float(eng.camera_reward_rows[idle].abs().sum()) == 0.0 and float(eng.target_reward_rows[idle].abs().sum()) == 0.0, s
        assert float(a.target_reward_terms[idle].abs().sum()) == 0.0
        assert bool((a.camera_reward_rows[~idle] >= 1.0).all()) and torch.equal(a.camera_reward_rows, b.camera_reward_rows), s
    assert idled > 0


# ---------------------------------------------------------------------------------------------- 6: graph replay
def test_graph_replay_accumulates_and_follows_the_coefficient_tensor():
    """A Stepper (versus = 'target', eight steps per graph, batched restarts every eighth) built after attaching: accumulating rows
    after one replay are the running sum of eight direct per-step calls on a twin, bit for bit, and an in-place write to
    reward_coefficients between two replays takes effect."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg, n = read_config('MATE-2v4-0.yaml'), 128
    coefficients = {'raw_reward': 1.0, 'coverage_rate': -1.0, 'normalized_goal_distance': -2.0, 'sparse_delivery': 100.0, 'is_tracked': -0.5}
    a, b = Engine(cfg, n, seed=37), Engine(cfg, n, seed=37)
    act = torch.linspace(-20.0, 20.0, n * 4 * 2, device='cuda', dtype=torch.float64).reshape(n, 4, 2).contiguous()
    for eng, accumulate in ((a, True), (b, False)):
        eng.enable_policies()
        eng.reset()
        eng.enable_reward_rows(target=(coefficients, 'none'), accumulate=accumulate)
    stepper = a.make_stepper(None, act, auto_reset=8, graph_steps=8, versus='target')
    assert stepper.target_reward_rows is a.target_reward_rows and stepper.warmup_steps == 8
    for _ in range(8):
        b.step_versus_greedy('target', act, auto_reset=8)
    totals = []
    for scale in (1.0, 3.0):
        for eng in (a, b):
            eng.reward_coefficients['target'].mul_(scale)
        a.target_reward_rows.zero_()
        stepper.run(8)
        total = torch.zeros_like(b.target_reward_rows)
        for _ in range(8):
            b.step_versus_greedy('target', act, auto_reset=8)
            total = total + b.target_reward_rows
        torch.cuda.synchronize()
        assert torch.equal(a.target_reward_rows, total), scale
        assert torch.equal(a.scalars, b.scalars)
        totals.append(total)
    assert float(totals[0].abs().sum()) > 0 and not torch.equal(totals[0], totals[1])
    stepper.close()


# ---------------------------------------------------------------------------------------------- 7: nothing else changes
def test_attaching_changes_no_other_output():
    """Observations, scalars, masks and the exported state of twenty steps (immediate restarts) are bit-identical with and without
    the rows attached."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-4v8-9.yaml', max_episode_steps=8)
    plain, shaped = Engine(cfg, 33, seed=41), Engine(cfg, 33, seed=41)
    for eng in (plain, shaped):
        eng.reset()
    shaped.enable_reward_rows(camera=({'coverage_rate': 1.0}, 'mean'), target=(dict(TARGET_COEFFICIENTS, soft_coverage_score=0.0), 'none'), terms=True)
    for s in range(20):
        for eng in (plain, shaped):
            eng.step_random(auto_reset=1, want_masks=True)
        for name in ('camera_obs', 'target_obs', 'scalars', 'masks'):
            assert torch.equal(getattr(plain, name), getattr(shaped, name)), (s, name)
        assert torch.equal(plain.export_state(), shaped.export_state()), s
    shaped.disable_reward_rows()
    assert shaped.target_reward_rows is None
    shaped.step_random(auto_reset=1, want_masks=False)      # detached: the masks are optional again


# ---------------------------------------------------------------------------------------------- 8: errors
def test_error_returns():
    from mate_amd._native import EngineError, MateRewardRows
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    eng = Engine(read_config('MATE-4v2-9.yaml'), 8, seed=43)
    with pytest.raises(EngineError, match='before reset') as err:
        eng.enable_reward_rows(target=({'baseline': 1.0}, 'none'))
    assert err.value.code == MATE_ESTATE
    eng.enable_policies()
    eng.reset()
    # soft coverage without the outer boundary, at the C level (Engine.enable_reward_rows would build it)
    rows, coef = torch.zeros((8, 4), dtype=torch.float64, device='cuda'), torch.zeros(7, dtype=torch.float64, device='cuda')
    cfg = MateRewardRows()
    cfg.camera_rows_dev, cfg.camera_coefficients_dev, cfg.out_dtype, cfg.soft_coverage = rows.data_ptr(), coef.data_ptr(), 1, 1
    assert eng.lib.mate_engine_enable_reward_rows(eng._h, ctypes.byref(cfg)) == MATE_ESTATE
    cfg.soft_coverage, cfg.camera_rows_dev = 0, rows.data_ptr() + 4
    assert eng.lib.mate_engine_enable_reward_rows(eng._h, ctypes.byref(cfg)) == MATE_EINVAL      # misaligned
    cfg.camera_rows_dev = None
    assert eng.lib.mate_engine_enable_reward_rows(eng._h, ctypes.byref(cfg)) == MATE_EINVAL      # no team at all
    eng.enable_reward_rows(target=({'baseline': 1.0}, 'none'))
    with pytest.raises(EngineError, match='masks_dev') as err:
        eng.step_random(auto_reset=1, want_masks=False)
    assert err.value.code == MATE_EINVAL
    with pytest.raises(EngineError, match='reward rows are attached') as err:
        eng.rollout_greedy(4, auto_reset='pipelined', want_masks=True)
    assert err.value.code == MATE_ESTATE
    eng.step_random(auto_reset=1, want_masks=True)
    assert bool((eng.target_reward_rows == 1.0).all())
    nav = Engine(read_config('MATE-Navigation.yaml'), 4, seed=44)
    nav.reset()
    with pytest.raises(EngineError, match='no cameras') as err:
        nav.enable_reward_rows(camera=({'baseline': 1.0}, 'none'))
    assert err.value.code == MATE_EINVAL
