"""GPU (-m gpu): _assign_goals (environment.py:1271-1324) on planted warehouse scenes in every launch form.

No random-policy trajectory of the suite reaches a warehouse (tests/test_logistics_scenes_cpu.py restates the census), so the step's
one order-dependent rule -- delivery, pick-up from the shared `remaining_cargoes` in index order, bounty decay, the empty bits, the
end of an episode by cargo -- ran in the greedy flows only, and never in the kernels that hold the targets' logistics in registers
(headline_rollout_kernel and rollout_kernel's HELDSTATE form: assign_and_score_held spills to the LDS record, runs the serial code on
lane 0 and reloads).  tests/logistics_scenes.py plants the rule's edges on natively reset batches of 22 environments (the catalogue is in
its docstring): neighbouring environments differ in whether any target is inside, so that a sub-wave kernel steps both in one wave.
tests/test_logistics_scenes_cpu.py shows with the oracle alone that every probe lands where the plan says and does what it expects.

Here every stepping entry point runs the plants, per shape, observation dtype, sub-wave mode, MATE_STEP_SPLIT (MATE-2v4-0),
MATE_HEADLINE_UNIT (the MATE-4v8-9 f32 cell: both fused random-policy kernels) and once with the sparse reward:
  step with f64 actions and see-through / goal tapes, step with f32 actions on the Philox draws, step_versus_greedy('target', action),
  rollout_versus_greedy('target', action, 3); with the probes' targets standing inside their warehouses step_greedy,
  step_versus_greedy('camera', 0), rollout_greedy(3), rollout_versus_greedy('camera', 0, 3); on the compensated plants (position =
  landing - the random policy's own draws) step_random and rollout_random(3); and, per cell, one compensated plant whose episode
  ends by cargo through rollout_random with immediate auto-reset and under a batched restart, and through step_random(auto_reset=1).
Where device agents act the oracle is fed the joint action the device chose (policy_actions() of the single-stepping twin; both
engines take every agent call, since the agents' memory is no part of the planted state).  Fused launches: byte for byte the single
steps of the twin while the episode runs (rows, masks, scalars, final state); behind its end the idle rows and the standing state.  Against
the oracle after every frame: the logistics state and scalar columns 0, 1, 2, 6 exact, the rates and the normalised reward 1e-6
(tests/test_gpu_reset_kat.py), positions 1e-9, target rows 1e-9 (f64) / 1e-5 * max(1, |ref|) (f32), the idle row behind an ended
episode whole; on the states tests/golden/kat_logistics.npz holds, against the reference's recorded outputs directly."""
import os

import numpy as np
import pytest
import torch

import gpu_util as U
import logistics_scenes as LS
import rim_scenes as RS
from launch_forms import GOLDEN, Matrix, recorded_flow, same

pytestmark = pytest.mark.gpu

FRAMES = LS.FRAMES
POSITION_TOL = 1e-9
RATE_TOL = 1e-6
IDLE_ROW = np.array([0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=np.float32)       # engine_kernels.hpp: write_idle_row
KAT = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kat_logistics.npz'))
KAT_ROWS = {(str(KAT['shapes'][s]), int(r), int(f), int(e)): i for i, (s, r, f, e) in enumerate(KAT['where'])}
# call of this file -> call of tools/launch_matrix.py CALL_LIST whose recorded [last_flow, sub_wave] it must run
RECORDED_CALL = {'step f32 drawn': 'step', 'step_versus_greedy target': 'step_versus_greedy_target', 'rollout_versus_greedy target': 'rollout_versus_greedy_target',
                 'step_greedy': 'step_greedy', 'step_versus_greedy camera': 'step_versus_greedy_camera', 'rollout_greedy': 'rollout_greedy',
                 'rollout_versus_greedy camera': 'rollout_versus_greedy_camera', 'step_random': 'step_random', 'rollout_random': 'rollout_random'}
CELLS = [(shape, dtype, split, '1', 'dense') for shape in LS.SHAPES for dtype in ('f32', 'f64') for split in (('0', '1') if shape == 'MATE-2v4-0' else ('0',))]
CELLS += [('MATE-4v8-9', 'f32', '0', '0', 'dense'), ('MATE-2v4-0', 'f32', '0', '1', 'sparse')]
FLOWS_SEEN = {}


def fail(where, env, what, plan):
    probes = LS.describe(LS.probes_at(plan, env)) or ['(no probe in this environment)']
    return '%s: environment %d (%s scene) %s differs; planted there: %s' % (where, env, LS.scene_kind(env), what, '; '.join(probes))


def check_frame(where, mx, eng, scalars, target_rows, live, plan):
    """The device behind a frame against the oracle behind the same frame, on the environments `live` [n] bool: those whose episode
    had not ended before the frame.  (With auto_reset = 0 the caller resets: what a step does to an ended episode is not part of the
    contract -- step() steps on, the flows on the rollout kernels idle -- and is compared nowhere.)"""
    side = mx.side
    sd, ref = eng.state_dict(), side.fields()
    for k in LS.LOGISTICS_KEYS:
        diff = (np.asarray(sd[k]).reshape(LS.BATCH, -1) != np.asarray(ref[k]).reshape(LS.BATCH, -1)).any(axis=1) & live
        if diff.any():
            e = int(np.flatnonzero(diff)[0])
            raise AssertionError(fail(where, e, '%s (device %s, oracle %s)' % (k, np.asarray(sd[k][e]).ravel().tolist(), np.asarray(ref[k][e]).ravel().tolist()), plan))
    err = np.maximum(np.abs(sd['tgt_x'] - ref['tgt_x']), np.abs(sd['tgt_y'] - ref['tgt_y'])).max(axis=1) * live
    if err.max() >= POSITION_TOL:
        raise AssertionError(fail(where, int(np.argmax(err)), 'position (off by %.3g)' % err.max(), plan))
    sc = scalars.cpu().numpy()
    want = LS.oracle_scalars(side)
    rows = target_rows.cpu().numpy().astype(np.float64)
    for e in np.flatnonzero(live):
        exact = [0, 1, 2, 6]
        if not np.array_equal(sc[e][exact], want[e][exact].astype(np.float32)):
            raise AssertionError(fail(where, e, 'scalars (camera reward, target reward, done, delivered): device %s, oracle %s' % (sc[e][exact].tolist(), want[e][exact].tolist()), plan))
        rates = [3, 4, 5, 7]
        if not np.all(np.abs(sc[e][rates].astype(np.float64) - want[e][rates]) < RATE_TOL):
            raise AssertionError(fail(where, e, 'scalars (coverage, real coverage, transport rate, normalised reward): device %s, oracle %s' % (sc[e][rates].tolist(), want[e][rates].tolist()), plan))
        ot = side.envs[e].observe()[1]
        bad = np.abs(rows[e] - ot) >= POSITION_TOL if mx.dtype == 'f64' else np.abs(rows[e] - ot) > 1e-5 * np.maximum(1.0, np.abs(ot))
        if bad.any():
            t, col = (int(v) for v in np.argwhere(bad)[0])
            raise AssertionError(fail(where, int(e), 'row of target %d, column %d (device %r, oracle %r)' % (t, col, rows[e][t, col], ot[t, col]), plan))


def check_kat(where, mx, eng, shape, rnd, frame, stepped, plan):
    """On the states kat_logistics.npz holds: the device behind the frame against what the reference's _assign_goals left (the counters
    one step() later: target_steps + 1, tracked_steps + tracked_bits) and its dense reward."""
    sd = eng.state_dict()
    sc = eng.scalars.cpu().numpy()
    Nt = mx.side.Nt
    hit = 0
    for e in np.flatnonzero(stepped):
        i = KAT_ROWS.get((shape, rnd, frame, int(e)))
        if i is None:
            continue
        hit += 1
        out = {k: KAT['out/' + k][i] for k in LS.LOGISTICS_KEYS[:10]}
        out['target_steps'] = out['target_steps'] + 1
        out['tracked_steps'] = out['tracked_steps'] + KAT['in/tracked_bits'][i]
        for k, v in out.items():
            v = v[:Nt] if k.startswith('tgt_') or v.shape[:1] == (8,) else v
            assert np.array_equal(np.asarray(sd[k][e], dtype=np.float64).ravel(), np.asarray(v, dtype=np.float64).ravel()), \
                fail(where + ' against the reference (%s)' % KAT['probes'][i], int(e), k, plan)
        reward = KAT['out/delayed_reward'][i] if mx.cfg['reward_type'] == 'sparse' else KAT['out/reward'][i]
        assert sc[e][1] == np.float32(reward) and sc[e][0] == np.float32(-reward), fail(where + ' against the reference', int(e), 'reward %r (recorded %r)' % (sc[e][1], reward), plan)
    return hit


def standing(scene, fields):
    """The scene with every probe's target standing inside its warehouse already (half way between its landing and the centre): under
    the on-device target agents, whose actions the plant does not choose, the logistics then run on frame 0 whatever they do."""
    out = {k: np.array(v, copy=True) for k, v in scene.state.items()}
    for p in scene.plan:
        if p.side < 0:
            out['tgt_x'][p.env, p.target], out['tgt_y'][p.env, p.target] = (np.asarray(p.landing) + LS.WAREHOUSES[p.warehouse]) / 2.0
    return out


def device(mx, array, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(array)).to(device=mx.a.device, dtype=dtype)


def first_difference(where, what, fused, stepped, live, plan):
    """Byte for byte on the environments `live`; a difference is named by environment, row and column."""
    x, y = (t.contiguous().reshape(LS.BATCH, -1).cpu().numpy() for t in (fused, stepped))
    diff = (x.view(np.uint8).reshape(LS.BATCH, -1) != y.view(np.uint8).reshape(LS.BATCH, -1)).any(axis=1) & live
    if diff.any():
        e = int(np.flatnonzero(diff)[0])
        cols = np.flatnonzero((x[e].view(np.uint8).reshape(x.shape[1], -1) != y[e].view(np.uint8).reshape(x.shape[1], -1)).any(axis=1))[:8]
        per_row = x.shape[1] // max(1, fused.shape[1]) if fused.dim() == 3 else x.shape[1]
        raise AssertionError(fail(where, e, '%s of the fused launch against the single step: (row, column, fused, single) %s'
                                  % (what, [(int(c // per_row), int(c % per_row), x[e][c].item(), y[e][c].item()) for c in cols]), plan))


def fused_against_twin(call, mx, launch, single, oracle, plan, frames=FRAMES, agents=True):
    """`launch(a)` -> rollout-shaped (camera rows, target rows, scalars) of engine a's fused call; `single(b)` steps the twin once;
    `oracle(b, live)` steps the oracle's running episodes on what the twin just did.  With auto_reset = 0 an environment whose episode
    ends stops inside a fused launch (idle rows, its state stands: include/mate_engine.h) while what single steps do to it is not
    part of the contract.  So: byte for byte, and the twin against the oracle, while the episode runs; behind its end the fused
    launch's idle rows and, at last, its state against the oracle's at the frame that ended the episode.
    `agents`: on-device agents act.  Their memory is no part of the planted state, and behind an episode's end the twin's agents go on
    where the fused launch's stop: from then on (mx.clean) the two engines' agents may choose differently in that environment, which is
    then compared on the twin alone."""
    a, b, side = mx.a, mx.b, mx.side
    cam_r, tgt_r, sc_r = launch(a)
    live = np.ones(LS.BATCH, dtype=bool)
    clean = mx.clean.copy() if agents else live.copy()
    at_end = {}
    for f in range(frames):
        single(b)
        where = '%s: frame %d' % (call, f)
        oracle(b, live)
        check_frame('%s frame %d (single steps of the twin)' % (call, f), mx, b, b.scalars, b.target_obs, live, plan)
        check_frame('%s frame %d (the fused launch; state of the twin)' % (call, f), mx, b, sc_r[f], tgt_r[f], live & clean, plan)
        for what, fused, stepped in (('scalars', sc_r[f], b.scalars), ('target rows', tgt_r[f], b.target_obs), ('camera rows', cam_r[f], b.camera_obs),
                                     ('masks', a._rollout['masks'][f], b.masks)):
            first_difference(where, what, fused, stepped, live & clean, plan)
        idle = sc_r[f][torch.from_numpy(~live).to(a.device)].cpu().numpy()
        assert np.array_equal(idle, np.broadcast_to(IDLE_ROW, idle.shape)), fail(where, int(np.flatnonzero(~live)[0]), 'idle scalar rows %s' % idle.tolist(), plan)
        done = side.batch.gather('done') != 0
        if (done & live).any():
            ref = side.fields()
            for e in np.flatnonzero(done & live & clean):
                at_end[int(e)] = {k: np.array(ref[k][e], copy=True) for k in LS.LOGISTICS_KEYS + ('tgt_x', 'tgt_y')}
        live &= ~done
    ran = torch.from_numpy(live & clean).to(a.device)
    assert same(a.export_state()[ran], b.export_state()[ran]), call + ': final state differs from the single steps'
    sd = a.state_dict()
    for e, ref in at_end.items():
        for k in LS.LOGISTICS_KEYS:
            assert np.array_equal(np.asarray(sd[k][e]).ravel(), ref[k].ravel()), fail(call + ' state behind the episode\'s end', e, k, plan)
        assert max(abs(sd['tgt_x'][e] - ref['tgt_x']).max(), abs(sd['tgt_y'][e] - ref['tgt_y']).max()) < POSITION_TOL, fail(call + ' state behind the episode\'s end', e, 'position', plan)
    if agents:
        mx.clean &= live
    return at_end


def run_planted_scene(mx, scene, rnd, where, note, kat_shape):
    a, b, side = mx.a, mx.b, mx.side
    plan = scene.plan
    fields = RS.merged(mx.sd, scene.state)
    flat = mx.flat_of(scene.state)
    act64 = device(mx, scene.actions)
    act32 = device(mx, scene.actions, torch.float32)
    assert np.array_equal(act32.cpu().numpy().astype(np.float64), scene.actions)        # the walks are f32 values
    goal_u = device(mx, scene.goal_u)
    # step with f64 actions, no see-through draws, the goal tape: frame by frame
    everyone = np.ones(LS.BATCH, dtype=bool)
    side.load(fields)
    mx.plant(a, flat)
    hits = 0
    live = everyone.copy()
    for f in range(FRAMES):
        a.step(mx.zero_cam[torch.float64], act64, tape_ct=mx.no_draws, tape_goal=goal_u, auto_reset=False)
        note('step f64 taped', a)
        LS.oracle_step(side, scene.actions, scene.goal_u, live=live)
        call = where + ' step(0, action) with f64 actions and tapes, frame %d' % f
        check_frame(call, mx, a, a.scalars, a.target_obs, live, plan)
        if kat_shape and f < 2:
            hits += check_kat(call, mx, a, mx.shape, rnd, f, live, plan)
        live &= side.batch.gather('done') == 0
    assert not kat_shape or rnd >= 2 or hits >= 30, (where, 'rows of kat_logistics.npz met', hits)
    # step with f32 actions: see-through draws and goal picks off the Philox stream both sides share
    side.load(fields)
    mx.plant(a, flat)
    live = everyone.copy()
    for f in range(2):
        a.step(mx.zero_cam[torch.float32], act32, auto_reset=False)
        note('step f32 drawn', a)
        LS.oracle_step(side, scene.actions, None, draws=True, live=live)
        check_frame(where + ' step(0, action) with f32 actions, drawn, frame %d' % f, mx, a, a.scalars, a.target_obs, live, plan)
        live &= side.batch.gather('done') == 0
    # step_versus_greedy('target', action) / rollout_versus_greedy('target', action, 3): the cameras are the device's agents
    def cameras_then_oracle(eng, live=None):
        LS.oracle_step(side, scene.actions, None, cam_act=eng.policy_actions()[0].cpu().numpy(), draws=True, live=live)

    side.load(fields)
    for eng in (a, b):      # (both: the agents' memory moves with every call they act in, and the twin's must stay the fused engine's)
        mx.plant(eng, flat)
        eng.step_versus_greedy('target', act32, auto_reset=False)
    note('step_versus_greedy target', a)
    cameras_then_oracle(a)
    check_frame(where + " step_versus_greedy('target', action)", mx, a, a.scalars, a.target_obs, everyone, plan)
    side.load(fields)
    for eng in (a, b):
        mx.plant(eng, flat)
    fused_against_twin(where + " rollout_versus_greedy('target', action, %d)" % FRAMES, mx,
                       lambda eng: eng.rollout_versus_greedy('target', act32, FRAMES, auto_reset=False, want_masks=True),
                       lambda eng: eng.step_versus_greedy('target', act32, auto_reset=False), cameras_then_oracle, plan)
    note('rollout_versus_greedy target', a)
    # the on-device target agents: the probes' targets stand in their warehouses
    inside = standing(scene, fields)
    fields_in, flat_in = RS.merged(mx.sd, inside), mx.flat_of(inside)

    def both_then_oracle(eng, live=None):
        cam_act, tgt_act = (x.cpu().numpy() for x in eng.policy_actions())
        LS.oracle_step(side, tgt_act, None, cam_act=cam_act, draws=True, live=live)

    def targets_then_oracle(eng, live=None):          # (the caller's cameras keep still)
        LS.oracle_step(side, eng.policy_actions()[1].cpu().numpy(), None, draws=True, live=live)

    for name, step_once, launch in (
            ('step_greedy', lambda eng: eng.step_greedy(auto_reset=False), None),
            ('step_versus_greedy camera', lambda eng: eng.step_versus_greedy('camera', mx.zero_cam[torch.float32], auto_reset=False), None),
            ('rollout_greedy', lambda eng: eng.step_greedy(auto_reset=False), lambda eng: eng.rollout_greedy(FRAMES, auto_reset=False, want_masks=True)),
            ('rollout_versus_greedy camera', lambda eng: eng.step_versus_greedy('camera', mx.zero_cam[torch.float32], auto_reset=False),
             lambda eng: eng.rollout_versus_greedy('camera', mx.zero_cam[torch.float32], FRAMES, auto_reset=False, want_masks=True))):
        if name.endswith('camera') and not a.num_cameras:
            continue
        side.load(fields_in)
        call = '%s %s, targets standing inside' % (where, name)
        then_oracle = targets_then_oracle if name.endswith('camera') else both_then_oracle
        if launch is None:
            for eng in (a, b):
                mx.plant(eng, flat_in)
                step_once(eng)
            then_oracle(a)
            check_frame(call, mx, a, a.scalars, a.target_obs, everyone, plan)
        else:
            for eng in (a, b):
                mx.plant(eng, flat_in)
            fused_against_twin(call, mx, launch, step_once, then_oracle, plan)
        note(name, a)


def check_restarted(where, mx, eng, envs, plan):
    """Environments `envs` of the engine hold the first state of their next episode: the oracle's own reset() of them, every state key."""
    sd = eng.state_dict()
    for e in envs:
        env = mx.side.envs[e]
        env.reset()
        for k in U.STATE_KEYS + ['episode']:
            assert np.array_equal(np.asarray(sd[k][e], dtype=np.float64).ravel(), np.asarray(env.get(k), dtype=np.float64).ravel()), fail(where + ' behind the restart', int(e), k, plan)
        assert sd['episode'][e] == mx.sd['episode'][e] + 1, fail(where + ' behind the restart', int(e), 'episode counter', plan)
    mx.side.set_tables(mx.tables)       # (the oracle's reset built tables of its own)


def run_restarts(mx, scene, draws, where):
    """Across an episode that ends by cargo, on a compensated plant under the random policy (no agent has a memory to keep in step).
    A fused launch stops the environment at the end of its episode and restarts it behind the launch (auto_reset = 1) or behind the
    second of two launches (a batched restart, auto_reset = 2): the frames up to the end against the oracle, with the state of a twin
    that single-steps; idle rows from there on; then the state of a natively reset episode.  Single steps with auto_reset = 1 restart
    inside the call that ends the episode."""
    a, b, side = mx.a, mx.b, mx.side
    plan = scene.plan
    fields, flat = RS.merged(mx.sd, scene.state), mx.flat_of(scene.state)
    ends = [p for p in plan if p.kind == 'end' and p.rung == 'last']
    assert ends, where

    def oracle(frame, live):
        LS.oracle_step(side, draws[frame][1].astype(np.float64), None, cam_act=draws[frame][0].astype(np.float64), draws=True, live=live)

    def replant(eng):
        """A restart built the occlusion tables of the new episode's obstacles: the plant needs those of its own again."""
        eng.import_state(flat)
        eng.rebuild_luts()
        eng.observe()
        for e in (p.env for p in ends):
            for c in range(eng.num_cameras):
                assert all(np.array_equal(x, y) for x, y in zip(eng.lut_read(e, c), mx.tables[e][c])), (where, 'rebuilt table', e, c)

    for auto_reset in (1, 2):
        for eng in (a, b):
            replant(eng)
        side.load(fields)
        live = np.ones(LS.BATCH, dtype=bool)
        call = '%s rollout_random(%d, auto_reset=%d)' % (where, FRAMES, auto_reset)
        for launch in range(auto_reset):
            cam_r, tgt_r, sc_r = a.rollout_random(FRAMES, auto_reset=auto_reset, want_masks=True)
            for f in range(FRAMES):
                b.step_random(auto_reset=False, want_masks=True)
                at = '%s launch %d frame %d' % (call, launch, f)
                oracle(launch * FRAMES + f, live)
                check_frame(at + ' (single steps of the twin)', mx, b, b.scalars, b.target_obs, live, plan)
                check_frame(at + ' (the fused launch; state of the twin)', mx, b, sc_r[f], tgt_r[f], live, plan)
                idle = sc_r[f][torch.from_numpy(~live).to(a.device)].cpu().numpy()
                assert np.array_equal(idle, np.broadcast_to(IDLE_ROW, idle.shape)), fail(at, int(np.flatnonzero(~live)[0]), 'idle scalar rows %s' % idle.tolist(), plan)
                live &= side.batch.gather('done') == 0
        assert all(not live[p.env] for p in ends), call
        ran = torch.from_numpy(live).to(a.device)
        assert same(a.export_state()[ran], b.export_state()[ran]), call + ': final state differs from the single steps'
        check_restarted(call, mx, a, np.flatnonzero(~live), plan)
    # single steps, restarted in the call that ends the episode (the scalars still describe the finished step)
    replant(a)
    side.load(fields)
    live = np.ones(LS.BATCH, dtype=bool)
    for f in range(FRAMES):
        a.step_random(auto_reset=True, want_masks=True)
        at = '%s step_random(auto_reset=1) frame %d' % (where, f)
        oracle(f, live)
        sc, want = a.scalars.cpu().numpy(), LS.oracle_scalars(side)
        for e in range(LS.BATCH):
            if live[e]:
                assert np.array_equal(sc[e][[0, 1, 2, 6]], want[e][[0, 1, 2, 6]].astype(np.float32)), fail(at, e, 'scalars %s, oracle %s' % (sc[e].tolist(), want[e].tolist()), plan)
            else:
                assert sc[e][2] == 0.0 and sc[e][6] == 0.0, fail(at, e, 'scalars of the restarted episode %s' % sc[e].tolist(), plan)
        done = side.batch.gather('done') != 0
        check_restarted(at, mx, a, np.flatnonzero(done & live), plan)
        live &= ~done
    assert all(not live[p.env] for p in ends), where


def run_compensated_scene(mx, scene, draws, where, note):
    """The random-policy flows on the plant that lands on the policy's own draws."""
    a, b, side = mx.a, mx.b, mx.side
    plan = scene.plan
    flat = mx.flat_of(scene.state)
    fields = RS.merged(mx.sd, scene.state)

    def oracle(frame, live=None):
        LS.oracle_step(side, draws[frame][1].astype(np.float64), None, cam_act=draws[frame][0].astype(np.float64), draws=True, live=live)

    side.load(fields)
    mx.plant(a, flat)
    a.step_random(auto_reset=False, want_masks=True)
    note('step_random', a)
    oracle(0)
    check_frame(where + ' step_random()', mx, a, a.scalars, a.target_obs, np.ones(LS.BATCH, dtype=bool), plan)
    side.load(fields)
    for eng in (a, b):
        mx.plant(eng, flat)
    frame = iter(range(FRAMES))
    fused_against_twin(where + ' rollout_random(%d)' % FRAMES, mx, lambda eng: eng.rollout_random(FRAMES, auto_reset=False, want_masks=True),
                       lambda eng: eng.step_random(auto_reset=False, want_masks=True), lambda eng, live: oracle(next(frame), live), plan, agents=False)
    note('rollout_random', a)


@pytest.mark.parametrize('shape,dtype,split,unit,reward', CELLS, ids=['-'.join(c[:2]) + '-split%s-unit%s-%s' % c[2:] for c in CELLS])
def test_goal_logistics_in_every_launch_form(shape, dtype, split, unit, reward, oracle_lib, monkeypatch):
    if shape == 'MATE-2v4-0':
        monkeypatch.setenv('MATE_STEP_SPLIT', split)            # (both read when an engine is created)
    monkeypatch.setenv('MATE_HEADLINE_UNIT', unit)
    cfg = RS.config_of(shape)
    if reward != 'dense':
        cfg = dict(cfg, reward_type=reward)
    unrecorded = []
    for mode in (False, True):
        mx = Matrix(shape, dtype, oracle_lib, cfg)          # (per mode: fresh agents)
        if mode and mx.a.set_sub_wave(True) <= 1:
            for eng in (mx.a, mx.b):
                eng.close()
            break
        for eng in (mx.a, mx.b):
            eng.set_sub_wave(mode)
        mx.clean = np.ones(LS.BATCH, dtype=bool)
        scenes = LS.build_scenes(mx.sd, mx.tables, mx.cfg, LS.SEED, LS.ROUNDS[shape])
        tick = int(mx.sd['tick'][0])
        draws = [mx.side.random_actions(tick + k) for k in range(FRAMES)]
        compensated = LS.build_scenes(mx.sd, mx.tables, mx.cfg, LS.SEED + 1, LS.ROUNDS[shape], draws=draws[:2])
        kat_shape = shape in [str(s) for s in KAT['shapes']]

        def note(call, eng):
            got = [eng.last_flow, eng.sub_wave]
            want = recorded_flow(shape, dtype, mode, split, call, RECORDED_CALL) if reward == 'dense' else None
            if want is not None and got != want and (mode, call, got, want) not in unrecorded:
                unrecorded.append((mode, call, got, want))
            FLOWS_SEEN[(shape, dtype, mode, split, unit, reward, call)] = got

        form = '%s %s obs sub_wave=%s MATE_STEP_SPLIT=%s MATE_HEADLINE_UNIT=%s %s reward' % (shape, dtype, mode, split, unit, reward)
        for r, scene in enumerate(scenes):
            run_planted_scene(mx, scene, r, '%s plant %d' % (form, r), note, kat_shape)
        for r, scene in enumerate(compensated):
            run_compensated_scene(mx, scene, draws, '%s compensated plant %d' % (form, r), note)
        for eng in (mx.a, mx.b):
            eng.close()
    assert not unrecorded, (shape, dtype, split, '(sub-wave mode, call, [last_flow, sub_wave] it ran, recorded)', unrecorded)


@pytest.mark.parametrize('shape,dtype,split,unit,reward', CELLS, ids=['-'.join(c[:2]) + '-split%s-unit%s-%s' % c[2:] for c in CELLS])
def test_restarts_across_an_episode_that_ends_by_cargo(shape, dtype, split, unit, reward, oracle_lib, monkeypatch):
    if shape == 'MATE-2v4-0':
        monkeypatch.setenv('MATE_STEP_SPLIT', split)
    monkeypatch.setenv('MATE_HEADLINE_UNIT', unit)
    cfg = RS.config_of(shape)
    if reward != 'dense':
        cfg = dict(cfg, reward_type=reward)
    mx = Matrix(shape, dtype, oracle_lib, cfg)
    tick = int(mx.sd['tick'][0])
    draws = [mx.side.random_actions(tick + k) for k in range(2 * FRAMES)]
    scenes = LS.build_scenes(mx.sd, mx.tables, mx.cfg, LS.SEED + 1, LS.ROUNDS[shape], draws=draws[:2])
    ending = [(-p.frame, r) for r, scene in enumerate(scenes) for p in scene.plan if p.kind == 'end' and p.rung == 'last']
    r = min(ending)[1]          # (on frame 1 of 3 where a target's draws allow it)
    for mode in [False] + ([True] if mx.a.set_sub_wave(True) > 1 else []):
        for eng in (mx.a, mx.b):
            eng.set_sub_wave(mode)
        run_restarts(mx, scenes[r], draws, '%s %s obs sub_wave=%s MATE_STEP_SPLIT=%s MATE_HEADLINE_UNIT=%s %s reward compensated plant %d' % (shape, dtype, mode, split, unit, reward, r))
    for eng in (mx.a, mx.b):
        eng.close()


def test_the_matrix_ran_the_flows_recorded_for_its_calls():
    """Over the matrix above (this test reads what it noted, so it runs behind it): on each recorded shape the (call, flow,
    environments per wave) seen are those tests/golden/launch_flows.json lists for these calls with set_sub_wave(False) and (True)."""
    from launch_forms import CALL_ORDER
    recorded_shapes = [s for s in LS.SHAPES if s in GOLDEN['flows']]
    assert len(recorded_shapes) == 5
    assert {key[:2] + key[3:6] for key in FLOWS_SEEN} == set(CELLS), 'run behind the whole matrix of this file (every cell notes its flows when it passes)'
    for shape in recorded_shapes:
        for dtype in ('f32', 'f64'):
            seen = {(call, tuple(v)) for (s, d, mode, split, unit, reward, call), v in FLOWS_SEEN.items() if s == shape and d == dtype and reward == 'dense' and call in RECORDED_CALL}
            listed = set()
            for mode in (False, True):
                row = GOLDEN['flows'][shape]['%s %s plain sub_wave=%s' % (shape, dtype, mode)]
                listed |= {(call, tuple(row[CALL_ORDER.index(name)][:2])) for call, name in RECORDED_CALL.items()}
            assert seen == listed, (shape, dtype, 'seen and not listed', sorted(seen - listed), 'listed and not seen', sorted(listed - seen))
