"""The attached launches (selection_kernel, reward_rows_kernel, fragment_rows_kernel, heuristic_drift_kernel, state_rows_kernel) and the
fused observation modes at the entity counts of tests/shape_edges.py ATTACHED_CASES, on the generic kernels.

camera_target_view_mask starts at bit 0 of an environment's mask words and camera c's row is bits c * Nt .. c * Nt + Nt - 1.  Every
shipped scenario has Nt in {1, 2, 4, 8}: no row crosses a 32-bit word, so the second-word branch of view_row (csrc/attached_tile.hpp) and
its callers never met a reference there.  7v5-3, 16v15-3 and 5v7-0 have rows that do; tests/test_shape_edges_cpu.py shows with the
oracle alone that those rows have seen targets on both sides of the boundary at once, and every test here counts the same from
Engine.unpack_masks() -- the host-side bit unpack the references read -- for the flow it runs.

References, all independent of the kernels under test: the NumPy restatements of tests/test_selection_host.py and _track_batch of
tests/test_gpu_selection.py on the exported state and the unpacked masks; the oracle's Env.state() and Env.observe_mode().  The
reward rows and the Heuristic opponent at these cases are further parameters of tests/test_gpu_reward_rows.py and
tests/test_gpu_heuristic.py.  With view_row cut to its first word the selection and fragment tests of the straddling cases fail here
and no earlier test does (profiles/HISTORY.md); reward_rows_kernel reads its rows bit by bit (view_bit) and is out of that mutation's reach.  Bars: f64 1e-9, f32 rows 1e-5 * max(1, |ref|), masks, rewards, metrics, action masks, integer sums: exact."""
import numpy as np
import pytest
import torch

import shape_edges as S
from test_gpu_parity import MASKS
from test_gpu_selection import TOL, _bits_of, _constants_of, _track_batch
from test_gpu_shape_edges import THREADS, _engine_and_oracle
from test_gpu_state_rows import _blocks_equal_observations
from test_selection_host import action_mask_numpy, metrics_numpy

pytestmark = pytest.mark.gpu
EINVAL = -1
SENTINEL = 12345.0


def _engine(case, policies=True, **kw):
    from mate_amd.engine import Engine
    eng = Engine(S.case_scenario(case), case.n, seed=case.seed, first_env_index=case.first, **kw)
    assert (eng.num_cameras, eng.num_targets, eng.num_obstacles) == case.shape and not eng.specialised
    assert eng.layout.bit_camera_target == 0
    if policies:
        eng.enable_policies()
    return eng


class _Straddle:
    """Frames per straddling row, added up over the views a test's references read."""

    def __init__(self, nc, nt):
        self.frames = {c: 0 for c in S.straddling_rows(nc, nt)}

    def add(self, view, keep=None):
        for c, n in S.straddling_frames(view if keep is None else view[keep]).items():
            self.frames[c] += n

    def check(self, what):
        if self.frames:
            print(what, 'frames per straddling row', self.frames)
            assert min(self.frames.values()) >= 1, (what, self.frames)


# ------------------------------------------------------------------ a. selection
@pytest.mark.parametrize('name,multi', [('7v5-3', True), ('7v5-3', False), ('16v15-3', True), ('5v7-0', True), ('16v16-9', True)])
def test_selection_on_rows_that_cross_words(name, multi):
    """test_batches_that_do_not_fill_their_tiles on the attached cases: twelve step_selected(auto_reset=True) calls on random selections,
    the executor against _track_batch on the state and the view exported before each step (1e-9; a camera-frame is left out only if the
    NumPy side's branch margin is below 1e-9 relative, at most 0.1 % of them), the metrics and the action mask exact against
    metrics_numpy / action_mask_numpy on the unpacked masks."""
    from mate_amd.engine import decode_selection
    case = S.attached_case(name)
    eng = _engine(case)
    eng.reset()
    eng.enable_selection(multi)
    n, Nc, Nt = case.n, eng.num_cameras, eng.num_targets
    consts = _constants_of(eng)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(case.seed)
    left_out, total, worst = 0, 0, 0.0
    straddle = _Straddle(Nc, Nt)
    assert np.array_equal(eng.action_mask.cpu().numpy(), action_mask_numpy(eng.unpack_masks()['camera_target_view_mask'], multi))
    for step in range(12):
        if multi:
            keep = torch.rand((n, Nc, Nt), device='cuda', generator=gen) < 0.45
            eng.selection.copy_(eng.encode_selection(keep.to(torch.int32)))
            sel = _bits_of(eng.selection.cpu().numpy(), Nt)
            assert np.array_equal(sel, keep.cpu().numpy())
        else:
            eng.selection.copy_(torch.randint(0, Nt + 1, (n, Nc), device='cuda', generator=gen, dtype=torch.int32))
            sel = decode_selection(eng.selection.cpu(), False, Nt).numpy()
            assert (sel.sum(axis=-1) <= 1).all() and sel.any() and not sel.any(axis=-1).all()
        sd = eng.state_dict()
        view = eng.unpack_masks()['camera_target_view_mask']
        straddle.add(view)
        expect, margins = _track_batch(sd, view, sel, consts)
        eng.step_selected(auto_reset=True)
        got = eng.selection_actions.cpu().numpy()
        use = margins >= 1e-9
        left_out += int((~use).sum())
        total += use.size
        worst = max(worst, float(np.abs(got - expect)[use].max()))
        assert worst <= TOL, (step, worst)
        done = eng.scalars[:, 2].cpu().numpy()
        after = eng.unpack_masks()['camera_target_view_mask']
        own = (done != 2) & (done != 1)                # (restarted inside the call: the masks are the new episode's)
        straddle.add(after, own)
        assert np.array_equal(eng.selection_metrics.cpu().numpy()[own], metrics_numpy(sel, after)[own]), step
        assert np.array_equal(eng.action_mask.cpu().numpy(), action_mask_numpy(after, multi)), step
        assert own.any()
    print(f'{name} {"multi" if multi else "single"} x {n}: worst executor error {worst:.3e}, {left_out} of {total} camera-frames left out')
    assert left_out <= 0.001 * total, (left_out, total)
    straddle.check(f'{name} step_selected {"multi" if multi else "single"}')


@pytest.mark.parametrize('mode', ['shared', 'enhanced'])
def test_team_observation_modes_on_sixteen_cameras(mode):
    """test_team_observation_modes_act_on_the_flag_column on 16v15-3: under SharedFieldOfView the executor's view is the OR of sixteen rows,
    seven of which cross a word, folded by a butterfly over all sixteen lanes of a group."""
    from mate_amd import constants as consts
    case = S.attached_case('16v15-3')
    eng = _engine(case, policies=False, obs_dtype=torch.float64)
    eng.set_obs_mode(camera=mode)
    eng.enable_policies()
    eng.reset()
    eng.enable_selection(True)
    n, Nc, Nt = case.n, eng.num_cameras, eng.num_targets
    column = consts.camera_observation_slices_of(Nc, Nt, eng.num_obstacles)['opponent_mask']
    gen = torch.Generator(device='cuda')
    gen.manual_seed(2)
    straddle = _Straddle(Nc, Nt)
    for step in range(8):
        eng.selection.copy_(torch.randint(0, 1 << Nt, (n, Nc), device='cuda', generator=gen, dtype=torch.int32))
        flags = eng.camera_obs[:, :, column].cpu().numpy() != 0
        view = eng.unpack_masks()['camera_target_view_mask']
        straddle.add(view)
        if mode == 'enhanced':
            assert flags.all()
        else:
            assert np.array_equal(flags, np.broadcast_to(view.any(axis=1, keepdims=True), flags.shape))
            assert not flags.all() and flags.any()
        assert np.array_equal(eng.action_mask.cpu().numpy(), action_mask_numpy(flags, True))
        sel = _bits_of(eng.selection.cpu().numpy(), Nt)
        expect, margins = _track_batch(eng.state_dict(), flags, sel, _constants_of(eng))
        eng.step_selected(auto_reset=False)
        assert np.abs(eng.selection_actions.cpu().numpy() - expect)[margins >= 1e-9].max() <= TOL
        after = eng.camera_obs[:, :, column].cpu().numpy() != 0
        assert np.array_equal(eng.selection_metrics.cpu().numpy(), metrics_numpy(sel, after))
    if mode == 'shared':                     # (under EnhancedObservation the view is all ones whatever the rows hold)
        straddle.check('16v15-3 step_selected under shared')


# ------------------------------------------------------------------ c. fragment rows on planted masks
@pytest.mark.parametrize('name', ['7v5-3', '16v15-3'])
def test_fragment_rows_on_planted_masks(name):
    """Engine.fragment_rows over K = 3 frames of step_random rows and scalars with mask words of uniformly random bits -- every row pattern
    on both sides of every word boundary occurs -- and the staggered done = 2 pattern of test_generic_shape_with_a_ragged_row.  The
    expected shaped rows are reward_rows.hpp's arithmetic (the terms in table order, product then add, summed in frame order) on
    unpack_masks(masks=frame words): 1e-9 with a second, mask-free term beside the mask term, exact with the mask term alone."""
    case = S.attached_case(name)
    eng = _engine(case, policies=False)
    eng.reset()
    N, K, Nc, Nt, dev = case.n, 3, eng.num_cameras, eng.num_targets, eng.device
    rows, scalars = {'camera': [], 'target': []}, []
    for f in range(K):
        eng.step_random(auto_reset=False)
        rows['camera'].append(eng.camera_obs.clone())
        rows['target'].append(eng.target_obs.clone())
        scalars.append(eng.scalars.clone())
    scalars = torch.stack(scalars)
    gen = torch.Generator(device='cpu').manual_seed(case.seed)
    masks = torch.randint(-2 ** 31, 2 ** 31, (K, N, eng.layout.mask_words), generator=gen, dtype=torch.int64).to(torch.int32).to(dev)
    last = torch.arange(N, device=dev) % (K + 1) - 1            # -1: no frame ran; else the last live frame
    for f in range(K):
        scalars[f, :, 2] = torch.where(last >= f, torch.zeros(N, device=dev), torch.full((N,), 2.0, device=dev))
    ran, live = (last >= 0).cpu().numpy(), (last[None, :] >= torch.arange(K, device=dev)[:, None]).cpu().numpy()      # [N], [K, N]
    view = np.stack([eng.unpack_masks(masks=masks[f])['camera_target_view_mask'] for f in range(K)])                  # [K, N, Nc, Nt]
    straddle = _Straddle(Nc, Nt)
    straddle.add(view, live)
    sc = scalars.double().cpu().numpy()
    mask_term = {'camera': view.sum(axis=3).astype(np.float64), 'target': view.any(axis=2).astype(np.float64)}      # num_tracked [K, N, Nc] | is_tracked [K, N, Nt]
    # (the mask term and its coefficient, a mask-free term of the scalar record -- earlier in both coefficient tables --, its coefficient and column)
    plans = {'camera': ('num_tracked', 1.0, 'coverage_rate', 0.5, 3), 'target': ('is_tracked', -0.5, 'raw_reward', 1.0, 1)}
    for team, (mask_key, c_mask, free_key, c_free, column) in plans.items():
        A, D = (Nc, eng.camera_obs_dim) if team == 'camera' else (Nt, eng.target_obs_dim)
        team_rows = torch.stack(rows[team])
        picked = team_rows[last.clamp(min=0), torch.arange(N, device=dev)]
        for shaping in (({mask_key: c_mask, free_key: c_free}, 'none'), ({mask_key: 1.0}, 'none')):
            out = {'obs': torch.full((N, A, D), SENTINEL, dtype=eng.obs_dtype, device=dev), 'frames': torch.zeros(N, dtype=torch.int32, device=dev),
                   'shaped': torch.full((N, A), SENTINEL, dtype=torch.float64, device=dev)}
            eng.fragment_rows(team, team_rows, scalars, masks=masks, shaping=shaping, out=out)
            torch.cuda.synchronize()
            assert torch.equal(out['frames'].long(), last + 1), (team, 'frames')
            assert torch.equal(out['obs'][last >= 0], picked[last >= 0]) and bool((out['obs'][last < 0] == SENTINEL).all()), (team, 'last live frame')
            expect = np.zeros((N, A))
            for f in range(K):                      # frame order; per frame the free term (earlier in both tables), then the mask term
                shaped = np.zeros((N, A))
                if free_key in shaping[0]:
                    shaped = shaped + shaping[0][free_key] * sc[f, :, column][:, None]
                shaped = shaped + shaping[0][mask_key] * mask_term[team][f]
                expect = np.where(live[f][:, None], expect + shaped, expect)
            got = out['shaped'].cpu().numpy()
            assert not ran.all() and (got[~ran] == 0.0).all()
            err = float(np.abs(got - expect).max())
            print(f'{name} {team} fragment rows {sorted(shaping[0])}: worst error {err:.3e}')
            if free_key in shaping[0]:
                assert err <= 1e-9, (team, err)
            else:                                   # sums of small integers
                assert np.array_equal(got, expect), (team, np.argwhere(got != expect)[:4].tolist())
                assert expect.max() >= (2 if team == 'camera' else 1) * K
    straddle.check(f'{name} planted masks')


# ------------------------------------------------------------------ e. state rows
def _planned_tile(nc, nt, no, size):
    """plan_state_rows (csrc/engine_host.h) restated: environments per workgroup of state_rows_kernel for rows of `size`-byte elements."""
    up = lambda x: (x + 15) // 16 * 16  # noqa: E731
    sw, ni = 3 * nc + 3 * no + 1, nt * 5 + 26
    dw = 2 * nc + 2 * nt + 2 + (ni + 1) // 2
    s = 13 + 9 * nc + 14 * nt + 3 * no + 2 * nt + 16
    tile = 16
    while tile > 4 and up(tile * (sw + dw) * 8) + up(tile * s * size) > 40 * 1024:
        tile //= 2
    return tile, s


@pytest.mark.parametrize('case', S.ATTACHED_CASES, ids=S.case_id)
def test_state_rows_against_the_oracle_at_every_step(case, oracle_lib):
    """test_rows_against_the_oracle_at_every_step on the generic shapes: f64 rows == Env.state() (1e-9) for every environment at the reset
    and after each of twenty step(actions) calls with external f32 actions -- no cameras, no obstacles, tiles of 16, 8 and 4 environments,
    an odd row width whose partial last tile ends in the scalar tail store -- and on a second engine the f32 rows' camera and target blocks
    bit for bit the f32 observation rows' own."""
    from mate_amd.engine import Engine
    O = oracle_lib
    cfg, eng, batch = _engine_and_oracle(case, O, torch.float32)
    n, (Nc, Nt, No) = case.n, case.shape
    for size in (8, 4):
        tile, S_dim = _planned_tile(Nc, Nt, No, size)
        assert S_dim == eng.state_dim
        if case.shape == (7, 5, 3):          # the partial last tile ends off a 16-byte boundary: the scalar tail store runs
            assert tile == 16 and (n % tile) * S_dim * size % 16 != 0
        if case.shape == (16, 16, 64):
            assert tile == 4 and S_dim == 621
    eng.enable_state_rows(dtype=torch.float64)
    twin = Engine(cfg, n, seed=case.seed, first_env_index=case.first, obs_dtype=torch.float32)
    twin.reset()
    twin.enable_state_rows()
    assert not twin.specialised and twin.state.dtype == torch.float32 and eng.state.dtype == torch.float64
    envs = [batch.env(e) for e in range(n)]
    worst = 0.0

    def compare(where):
        nonlocal worst
        ref = np.stack([env.state() for env in envs])
        err = np.abs(eng.state.cpu().numpy() - ref)
        worst = max(worst, float(err.max()))
        assert np.all(err <= 1e-9), (where, float(err.max()), np.argwhere(err > 1e-9)[:4].tolist())
        _blocks_equal_observations(twin, where)

    compare('reset')
    rng = np.random.RandomState(case.seed)
    for s in range(20):
        ca = rng.uniform(-1.0, 1.0, (n, Nc, 2)).astype(np.float32) * np.float32(6.0)
        ta = rng.uniform(-1.0, 1.0, (n, Nt, 2)).astype(np.float32) * np.float32(25.0)
        for e in (eng, twin):
            e.step(torch.from_numpy(ca).cuda() if Nc else None, torch.from_numpy(ta).cuda(), auto_reset=False)
        assert eng.last_flow == 2             # the f32-actions compilation of the generic step kernel
        batch.step(ca if Nc else None, ta, auto_reset=False, threads=THREADS)
        compare(s)
    assert torch.equal(eng.scalars, twin.scalars) and torch.equal(eng.export_state(), twin.export_state())
    guard = torch.full((n * eng.state_dim + 8,), -7.0, dtype=torch.float32, device='cuda')      # nothing is written behind the array's end
    out = guard[:n * eng.state_dim].view(n, eng.state_dim)
    twin.state_rows(out=out)
    assert torch.equal(out, twin.state) and bool((guard[n * eng.state_dim:] == -7.0).all())
    print(f'{S.case_id(case)} x {n}: worst f64 state row error {worst:.3e}')


# ------------------------------------------------------------------ f. observation modes and external actions
@pytest.mark.parametrize('modes', [('shared', 'enhanced'), ('enhanced', 'shared')], ids='-'.join)
@pytest.mark.parametrize('name', ['7v5-3', '16v15-3'])
def test_observation_modes_under_external_actions(name, modes, oracle_lib):
    """test_observation_modes_vs_oracle_rollout on the generic kernels, stepped with Engine.step on seeded f32 actions: both teams' rows at
    every step against the oracle's restatement of the wrappers -- an f64-observation engine 1e-9, an f32 one 1e-5 * max(1, |ref|) --,
    all view masks and both rewards exact."""
    O = oracle_lib
    case = S.attached_case(name)
    cfg, eng64, batch = _engine_and_oracle(case, O, torch.float64, modes=modes)
    eng32 = _engine(case, policies=False)
    eng32.set_obs_mode(camera=modes[0], target=modes[1])
    eng32.reset()
    n, (Nc, Nt, _) = case.n, case.shape
    envs = [batch.env(e) for e in range(n)]
    worst = {'f64': 0.0, 'f32': 0.0}

    def rows(where):
        ref = [env.observe_mode(camera=modes[0], target=modes[1]) for env in envs]
        oc, ot = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
        for eng, key in ((eng64, 'f64'), (eng32, 'f32')):
            for got, want, team in ((eng.camera_obs, oc, 'camera rows'), (eng.target_obs, ot, 'target rows')):
                err = np.abs(got.double().cpu().numpy() - want)
                scale = 1.0 if key == 'f64' else np.maximum(1.0, np.abs(want))
                worst[key] = max(worst[key], float((err / scale).max()))
                bad = err > (1e-9 if key == 'f64' else 1e-5) * scale
                assert not bad.any(), (where, key, team, float(err.max()), np.argwhere(bad)[:4].tolist())

    rows('reset')
    rng = np.random.RandomState(case.seed + 1)
    straddle = _Straddle(Nc, Nt)
    for s in range(20):
        ca = rng.uniform(-1.0, 1.0, (n, Nc, 2)).astype(np.float32) * np.float32(6.0)
        ta = rng.uniform(-1.0, 1.0, (n, Nt, 2)).astype(np.float32) * np.float32(25.0)
        for eng in (eng64, eng32):
            eng.step(torch.from_numpy(ca).cuda(), torch.from_numpy(ta).cuda(), auto_reset=False)
            assert eng.last_flow == 0         # a team mode: the kernel that reads every switch
        batch.step(ca, ta, auto_reset=False, threads=THREADS)
        for eng in (eng64, eng32):
            masks = eng.unpack_masks()
            for m in MASKS:
                ref = batch.gather(m) != 0
                assert np.array_equal(masks[m].reshape(ref.shape), ref), (m, 'step', s)
            sc = eng.scalars.cpu().numpy()
            assert np.array_equal(sc[:, 0], batch.gather('reward_cam').astype(np.float32)), ('camera reward', 'step', s)
            assert np.array_equal(sc[:, 1], batch.gather('reward_tgt').astype(np.float32)), ('target reward', 'step', s)
        straddle.add(masks['camera_target_view_mask'])
        rows(('step', s))
    print(f'{name} {modes}: worst f64 row error {worst["f64"]:.3e}, worst f32 row error {worst["f32"]:.3e} of max(1, |ref|)')
    straddle.check(f'{name} step(actions) under {modes}')


# ------------------------------------------------------------------ g. no cameras
def test_no_cameras_refuse_the_camera_side_and_step_on():
    import ctypes
    from mate_amd._native import EngineError
    eng = _engine(S.attached_case('0v5-64'))
    eng.reset()
    before = eng.export_state().clone()
    with pytest.raises(EngineError, match='enable_selection') as err:
        eng.enable_selection(True)                    # (an empty selection tensor has no address: refused as a null buffer)
    assert err.value.code == EINVAL and eng.selection is None and eng.action_mask is None
    buf = torch.zeros(64, dtype=torch.float64, device=eng.device)
    ptr = ctypes.c_void_p(buf.data_ptr())
    assert eng.lib.mate_engine_enable_selection(eng._h, 1, ptr, ptr, ptr, ptr, 0) == EINVAL
    assert 'no cameras to act for' in eng.lib.mate_engine_last_error().decode()
    with pytest.raises(EngineError, match='no cameras to shape rewards for') as err:
        eng.enable_reward_rows(camera=({'baseline': 1.0}, 'none'))
    assert err.value.code == EINVAL and eng.camera_reward_rows is None
    assert torch.equal(before, eng.export_state())      # nothing ran
    eng.enable_reward_rows(target=({'baseline': 1.0, 'is_tracked': 1.0}, 'none'))
    eng.step_random(auto_reset=False, want_masks=True)
    eng.step_greedy(auto_reset=False)
    assert bool((eng.target_reward_rows == 1.0).all()) and not torch.equal(before, eng.export_state())
