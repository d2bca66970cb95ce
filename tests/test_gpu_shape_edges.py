"""The generic (AnyShape) kernels at the entity counts where they switch algorithm, and at the maxima include/mate_engine.h
promises (16 cameras, 16 targets, 64 obstacles): native reset + Philox random-policy rollout against the CPU oracle on the same
streams, compared at EVERY step and in EVERY environment -- all five view masks and the tracked bits, the integer state,
tgt_colliding, rewards: exact; positions and camera poses: 1e-9; f32 rows: 1e-5 * max(1, |ref|); the f64-observation engine's
rows: 1e-9; table knots 1e-9 up to the reference's own tangent-ray coin flips.  The scenarios, seeds, batches and step counts
come from tests/shape_edges.py; tests/test_shape_edges_cpu.py shows with the oracle alone that their targets run into the
camera bodies (those past the 64th circle where that is the point) more than a hundred times each.

On the kernels before the fix that came with this file (two 32-bit near words per target in the LDS form of
simulate_targets' screen, bit k - 32 set for a circle k >= 64) the two cases with more than 64 circles, 1v2-64 and 16v16-64,
failed on tgt_colliding at the first step a target walked into a camera: targets passed through the bodies of cameras
64 - No .. Nc - 1."""
import numpy as np
import pytest
import torch

import golden_util as G
import gpu_util as U
import shape_edges as S
from test_gpu_parity import INT_KEYS, MASKS

pytestmark = pytest.mark.gpu

F64_STATE = ('cam_phi', 'cam_theta', 'tgt_x', 'tgt_y')          # 1e-9; every other state key is exact
THREADS = 8
# a second, f64-observation engine where it is cheap (not the 16-camera batches: 1.5k-3k-knot tables read back per camera)
F64_CASES = [c for c in S.CASES if c.shape[0] < 16]
assert set(INT_KEYS) <= set(U.STATE_KEYS)        # the exact comparison of every state key but F64_STATE covers the integer state


def _engine_and_oracle(case, O, dtype, policies=False, modes=None):
    """Engine and oracle batch of a case on the same Philox seed and first_env_index, both reset; reset state exact, table knots
    1e-9 with only tangent-ray flips, then the device's tables on both sides.  `modes`: (camera, target) of set_obs_mode."""
    from mate_amd.engine import Engine
    cfg = S.case_scenario(case)
    eng = Engine(cfg, case.n, seed=case.seed, first_env_index=case.first, obs_dtype=dtype)
    assert (eng.num_cameras, eng.num_targets, eng.num_obstacles) == case.shape and not eng.specialised
    if modes is not None:
        eng.set_obs_mode(camera=modes[0], target=modes[1])
    if policies:
        eng.enable_policies()
    eng.reset()
    torch.cuda.synchronize()
    batch = S.oracle_batch(O, case, cfg)
    sd = eng.state_dict()
    for k in U.STATE_KEYS:
        ref = batch.gather(k)
        assert np.array_equal(sd[k].reshape(ref.shape), ref), ('reset', k)
    for e in range(case.n):
        oe = batch.env(e)
        obstacles = np.stack([sd['obs_x'][e], sd['obs_y'][e], sd['obs_radius'][e]], axis=-1)
        for c in range(eng.num_cameras):
            gp, gr = eng.lut_read(e, c)
            op, orr = oe.get_lut(c)
            assert len(gp) == len(op), (e, c, len(gp), len(op))
            assert np.abs(gp - op).max() < 1e-9, (e, c)
            G.assert_only_tangent_flips(gp, gr, orr, (sd['cam_x'][e][c], sd['cam_y'][e][c]), float(cfg['camera']['max_sight_range']), obstacles, 1e-6, (e, c))
            oe.set_lut(c, gp, gr)
    batch.update_view_reset()
    return cfg, eng, batch


def _check_rows(eng, batch, dtype, where):
    """Both teams' observation rows of every environment: f32 engine 1e-5 * max(1, |ref|) against the oracle's f32 rows, f64 engine
    1e-9 against its f64 rows."""
    n, Nc = eng.num_envs, eng.num_cameras
    co = eng.camera_obs.cpu().numpy() if Nc else None
    to = eng.target_obs.cpu().numpy()
    if dtype == torch.float32:
        oc, ot = batch.observe(threads=THREADS)
        bad = np.abs(to - ot) > 1e-5 * np.maximum(1.0, np.abs(ot))
        assert not bad.any(), (where, 'target rows', np.argwhere(bad)[:4].tolist(), float(np.abs(to - ot).max()))
        if Nc:
            bad = np.abs(co - oc) > 1e-5 * np.maximum(1.0, np.abs(oc))
            assert not bad.any(), (where, 'camera rows', np.argwhere(bad)[:4].tolist(), float(np.abs(co - oc).max()))
    else:
        for e in range(n):
            oc, ot = batch.env(e).observe()
            assert np.abs(to[e] - ot).max() < 1e-9, (where, e, 'target rows', float(np.abs(to[e] - ot).max()))
            if Nc:
                assert np.abs(co[e] - oc).max() < 1e-9, (where, e, 'camera rows', float(np.abs(co[e] - oc).max()))


def _rollout_vs_oracle(case, O, dtype):
    cfg, eng, batch = _engine_and_oracle(case, O, dtype)
    n = case.n
    _check_rows(eng, batch, dtype, 'reset')
    for s in range(case.steps):
        eng.step_random(auto_reset=False, want_masks=True)
        batch.step(auto_reset=False, threads=THREADS)
        sd = eng.state_dict()
        # (collisions first: what a skipped circle shows up in before anything else)
        ref = batch.gather('tgt_colliding')
        diff = sd['tgt_colliding'].reshape(ref.shape) != ref
        assert not diff.any(), ('tgt_colliding', 'step', s, '(environment, target)', np.argwhere(diff)[:6].tolist())
        for k in F64_STATE:
            ref = batch.gather(k)
            err = np.abs(sd[k].reshape(ref.shape) - ref)
            assert err.size == 0 or err.max() < 1e-9, (k, 'step', s, float(err.max()), np.argwhere(err >= 1e-9)[:6].tolist())
        masks = eng.unpack_masks()
        for m in MASKS:
            ref = batch.gather(m) != 0
            diff = masks[m].reshape(ref.shape) != ref
            assert not diff.any(), (m, 'step', s, np.argwhere(diff)[:6].tolist())
        for k in U.STATE_KEYS:
            if k in F64_STATE:
                continue
            ref = batch.gather(k)
            diff = sd[k].reshape(ref.shape) != ref
            assert not diff.any(), (k, 'step', s, np.argwhere(diff)[:6].tolist())
        sc = eng.scalars.cpu().numpy()
        assert np.array_equal(sc[:, 1], batch.gather('reward_tgt').astype(np.float32)), ('target reward', 'step', s)
        assert np.array_equal(sc[:, 0], batch.gather('reward_cam').astype(np.float32)), ('camera reward', 'step', s)
        _check_rows(eng, batch, dtype, ('step', s))


@pytest.mark.parametrize('case', S.CASES, ids=S.case_id)
def test_edge_shape_rollout_vs_oracle(case, oracle_lib):
    """The product dtype (f32 rows) on every case of the matrix."""
    _rollout_vs_oracle(case, oracle_lib, torch.float32)


@pytest.mark.parametrize('case', F64_CASES, ids=S.case_id)
def test_edge_shape_rollout_vs_oracle_f64_rows(case, oracle_lib):
    """... and the f64-observation build of the same kernels, rows to 1e-9."""
    _rollout_vs_oracle(case, oracle_lib, torch.float64)


@pytest.mark.parametrize('case', S.CASES, ids=S.case_id)
def test_edge_shape_fused_rollout_equals_single_steps(case):
    """rollout_random(K) == K x step_random(), bit for bit: rows, scalars, masks and the final state.  The fused random rollout
    runs in the LDS slice the step kernel has (an engine that could be created can launch it), so every case must fit; the steps
    are the first ones after the reset, when the targets stand beside the camera bodies."""
    from mate_amd.engine import Engine
    cfg = S.scenario(case.shape)
    K = 12
    a, b = (Engine(cfg, case.n, seed=case.seed, first_env_index=case.first) for _ in range(2))
    for e in (a, b):
        e.reset()
    for rnd in range(2):
        cam_r, tgt_r, sc_r = a.rollout_random(K, auto_reset=False, want_masks=True)
        for r in range(K):
            b.step_random(auto_reset=False, want_masks=True)
            assert torch.equal(sc_r[r], b.scalars), (rnd, r, 'scalars')
            assert torch.equal(tgt_r[r], b.target_obs), (rnd, r, 'target rows')
            if a.num_cameras:
                assert torch.equal(cam_r[r], b.camera_obs), (rnd, r, 'camera rows')
            assert torch.equal(a._rollout['masks'][r], b.masks), (rnd, r, 'masks')
        assert torch.equal(a.export_state(), b.export_state()), rnd


@pytest.mark.parametrize('case', S.GREEDY_CASES, ids=S.case_id)
def test_edge_shape_greedy_agents_vs_oracle(case, oracle_lib):
    """The on-device greedy agents at 9 cameras (81 (sender, recipient) pairs: the first shape with two message rounds) and at
    16 cameras and 16 targets (four rounds; `(1u << Nt) - 1u`): closed loop against the oracle's restatement of the reference
    agents on recorded draws -- joint actions 1e-8, masks / goals / bounties exact -- and, on Philox draws, the fused rollout
    against single steps where it fits the LDS (an EngineError that says so where it does not)."""
    from mate_amd._native import EngineError
    from mate_amd.engine import Engine
    O = oracle_lib
    cfg, eng, batch = _engine_and_oracle(case, O, torch.float32, policies=True)
    n, (Nc, Nt, _) = case.n, case.shape
    envs = [batch.env(e) for e in range(n)]
    agents = [O.GreedyPolicies() for _ in range(n)]
    rng = np.random.RandomState(case.seed)
    reset_u = rng.random_sample((n, Nt, 2))
    dev = eng.device
    worst = 0.0
    for s in range(case.steps):
        t = {'camera_resample_u': rng.random_sample((n, Nc)), 'camera_sample_u': rng.random_sample((n, Nc, 2)),
             'camera_delay': rng.randint(6, 50, size=(n, Nc, Nc)).astype(np.int32),
             'target_choice_u': rng.random_sample((n, Nt)), 'target_resample_u': rng.random_sample((n, Nt)),
             'target_sample_u': rng.random_sample((n, Nt, 2)), 'target_reset_sample_u': reset_u}
        tape_ct, goal_u = rng.random_sample((n, Nc, Nt)), rng.random_sample((n, Nt))
        eng.step_greedy(policy_tape={k: torch.from_numpy(v).to(dev) for k, v in t.items()}, tape_ct=torch.from_numpy(tape_ct).to(dev),
                        tape_goal=torch.from_numpy(goal_u).to(dev), auto_reset=False)
        cam_act, tgt_act = (a.cpu().numpy() for a in eng.policy_actions())
        for e in range(n):
            ca, ta = agents[e].act(envs[e], t['camera_resample_u'][e], t['camera_sample_u'][e], t['camera_delay'][e],
                                   t['target_choice_u'][e], t['target_resample_u'][e], t['target_sample_u'][e], reset_u[e])
            worst = max(worst, float(np.abs(ta - tgt_act[e]).max()), float(np.abs(ca - cam_act[e]).max()))
            envs[e].step(ca, ta, tape_ct[e], goal_u[e])
        assert worst < 1e-8, (s, worst)
        masks = eng.unpack_masks()
        assert np.array_equal(masks['camera_target_view_mask'], batch.gather('camera_target_view_mask').reshape(n, Nc, Nt) != 0), s
        sd = eng.state_dict()
        for k in ('tgt_goals', 'bounties', 'freights', 'num_delivered_cargoes', 'tgt_colliding'):
            ref = batch.gather(k)
            assert np.array_equal(sd[k].reshape(ref.shape), ref), (k, s)
        assert np.abs(sd['tgt_x'] - batch.gather('tgt_x')).max() < 1e-8 and np.abs(sd['tgt_y'] - batch.gather('tgt_y')).max() < 1e-8, s
    a, b = (Engine(cfg, case.n, seed=case.seed, first_env_index=case.first) for _ in range(2))
    for e in (a, b):
        e.enable_policies()
        e.reset()
    try:
        cam, tgt, sc = a.rollout_greedy(12, auto_reset=False)
    except EngineError as err:
        assert 'LDS' in str(err) and 'fit' in str(err), err
        print(S.case_id(case), 'fused greedy rollout refused:', err)
        return
    for r in range(12):
        b.step_greedy(auto_reset=False)
        assert torch.equal(cam[r], b.camera_obs) and torch.equal(tgt[r], b.target_obs) and torch.equal(sc[r], b.scalars), r
    assert torch.equal(a.export_state(), b.export_state())
