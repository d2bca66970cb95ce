"""GPU (-m gpu): the verdicts of Sensor.perceive, Camera.perceive and Target.simulate ON THEIR RIMS in every launch form.

tests/rim_scenes.py plants, on natively reset batches of 22 environments, targets on the range rims of other targets, cameras and
obstacles (the edges of the f32 band, 1e-5 ... 1e-12 either side, the nearest f64 point), camera poses that put another camera's
centre on the sector edge or the sight rim, targets on the sector-edge, sight and occlusion-lookup rims of a camera, and targets one
full step (+ radius) (1 + delta) in front of a circle with the action pointing at it -- on frame 0, and one step further out so that
the rim is met on frame 1 of a fused launch, where the collision screen is the one carried from frame 0's range tests (under the
random policy: where the Philox draw of frame 0 or 1 points at a circle).
tests/test_rim_scenes_cpu.py shows with the oracle alone that the probes stand where the plan says.  Here every stepping entry point
runs the plants, per shape (the specialised, sub-wave, two-round and compact-list kernels and a generic one), observation dtype,
sub-wave mode and MATE_STEP_SPLIT switch, against the oracle on the same state and the device's own occlusion tables.  A mask is
compared wherever the plant makes it a pure function of inputs both sides share; masks and integers exact, positions 1e-9 (the
project's figure, tests/test_gpu_shape_edges.py); the fused launches bit-identical to single steps on a twin engine."""
import numpy as np
import pytest
import torch

import rim_scenes as RS
from launch_forms import CALL_ORDER, GOLDEN, RECORDED_CALL, Matrix, recorded_flow, same

pytestmark = pytest.mark.gpu

FRAMES = 3
POSITION_TOL = 1e-9
FLOWS_SEEN = {}             # (shape, dtype, mode, split, call) -> [last_flow, sub_wave], filled by the matrix below


def oracle_frames(side, fields, actions, frames):
    """The oracle's masks, tgt_colliding and positions behind each of `frames` steps of the target action on the planted state."""
    side.load(fields)
    out = []
    for _ in range(frames):
        side.step(None, actions)
        out.append((side.masks(), side.batch.gather('tgt_colliding') != 0, side.batch.gather('tgt_x'), side.batch.gather('tgt_y')))
    return out


def fail(where, env, what, pair, plan):
    probes = RS.describe(RS.probes_at(plan, env)) or ['(no probe in this environment)']
    return '%s: environment %d (%s scene) %s %s differs from the oracle; planted there: %s' % (where, env, RS.scene_kind(env), what, pair, '; '.join(probes))


def check_masks(where, got, ref, names, plan, valid=None):
    """Masks of `names`, exact; `valid` [n, Nt]: the targets whose verdicts the plant still determines (rows and, for the target-target
    mask, columns of the others are left out)."""
    for m in names:
        diff = np.asarray(got[m]).reshape(ref[m].shape) != ref[m]
        if valid is not None and m in RS.TARGET_SIDE:
            diff &= valid[:, :, None]
            if m == 'target_target_view_mask':
                diff &= valid[:, None, :]
        if diff.any():
            e, i, j = (int(v) for v in np.argwhere(diff)[0])
            raise AssertionError(fail(where, e, m, (i, j), plan))


def check_targets(where, dev, ref_colliding, ref_x, ref_y, plan, valid=None):
    valid = np.ones(ref_colliding.shape, dtype=bool) if valid is None else valid
    diff = (dev['tgt_colliding'].reshape(ref_colliding.shape) != 0) != ref_colliding
    diff &= valid
    if diff.any():
        e, t = (int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(fail(where, e, 'tgt_colliding', (t,), plan))
    err = np.maximum(np.abs(dev['tgt_x'].reshape(ref_x.shape) - ref_x), np.abs(dev['tgt_y'].reshape(ref_y.shape) - ref_y)) * valid
    if err.max() >= POSITION_TOL:
        e, t = (int(v) for v in np.unravel_index(np.argmax(err), err.shape))
        raise AssertionError(fail(where, e, 'position (off by %.3g)' % err.max(), (t,), plan))


def run_planted_scene(mx, scene, where, note):
    """Every call on one plant.  `note(call, engine)` records the flow the call ran."""
    a, b, side = mx.a, mx.b, mx.side
    plan = scene.plan
    fields = RS.merged(mx.sd, scene.state)
    flat = mx.flat_of(scene.state)
    act32 = torch.from_numpy(scene.actions.astype(np.float32)).to(a.device)
    assert np.array_equal(act32.cpu().numpy().astype(np.float64), scene.actions)        # the touch actions are f32 values
    side.load(fields)
    side.update_view()
    view = side.masks()
    # observe()
    mx.plant(a, flat)
    a.observe(tape_ct=mx.no_draws)
    note('observe', a)
    check_masks(where + ' observe()', a.unpack_masks(), view, RS.MASKS, plan)
    # step(0, 0): nothing moves, the view is the planted one
    still = oracle_frames(side, fields, None, 1)[0]
    for name, d in (('f64', torch.float64), ('f32', torch.float32)):
        mx.plant(a, flat)
        a.step(mx.zero_cam[d], mx.zero_tgt[d], tape_ct=mx.no_draws, auto_reset=False)
        note('step ' + name, a)
        check_masks(where + ' step(0, 0) with %s actions' % name, a.unpack_masks(), still[0], RS.MASKS, plan)
    # ... and without a tape, the see-through draws from the Philox stream both sides share (the f32-actions flow takes no tape)
    side.load(fields)
    side.step(None, None, draws=True)
    mx.plant(a, flat)
    a.step(mx.zero_cam[torch.float32], mx.zero_tgt[torch.float32], auto_reset=False)
    note('step f32 drawn', a)
    check_masks(where + ' step(0, 0) with f32 actions, drawn see-through', a.unpack_masks(), side.masks(), RS.MASKS, plan)
    # step_versus_greedy('target', action): the target kinematics and the target-side masks do not depend on the greedy cameras
    frames = oracle_frames(side, fields, scene.actions, FRAMES)
    for eng in (a, b):
        mx.plant(eng, flat)
        eng.step_versus_greedy('target', act32, auto_reset=False)
    note('step_versus_greedy target', a)
    call = where + " step_versus_greedy('target', action)"
    check_masks(call, a.unpack_masks(), frames[0][0], RS.TARGET_SIDE, plan)
    check_targets(call, mx.device_state(a), *frames[0][1:], plan)
    # rollout_versus_greedy('target', action, 3) against the oracle frame by frame and against three single steps of the twin
    for eng in (a, b):
        mx.plant(eng, flat)
    cam_r, tgt_r, sc_r = a.rollout_versus_greedy('target', act32, FRAMES, auto_reset=False, want_masks=True)
    note('rollout_versus_greedy target', a)
    call = where + " rollout_versus_greedy('target', action, %d)" % FRAMES
    for f in range(FRAMES):
        b.step_versus_greedy('target', act32, auto_reset=False)
        assert same(sc_r[f], b.scalars) and same(tgt_r[f], b.target_obs) and same(cam_r[f], b.camera_obs), '%s: frame %d rows / scalars differ from the single step' % (call, f)
        assert same(a._rollout['masks'][f], b.masks), '%s: frame %d masks differ from the single step' % (call, f)
        valid = scene.valid_until >= f
        check_masks('%s frame %d' % (call, f), a.unpack_masks(a._rollout['masks'][f]), frames[f][0], RS.TARGET_SIDE, plan, valid)
        check_targets('%s frame %d (single steps of the twin)' % (call, f), mx.device_state(b), *frames[f][1:], plan, valid)
    assert same(a.export_state(), b.export_state()), call + ': final state differs from three single steps'
    check_targets(call + ' final state', mx.device_state(a), *frames[FRAMES - 1][1:], plan, scene.valid_until >= FRAMES - 1)
    # step_versus_greedy('camera', 0): the cameras keep their poses
    for eng in (a, b):
        mx.plant(eng, flat)
        eng.step_versus_greedy('camera', mx.zero_cam[torch.float32], auto_reset=False)
    note('step_versus_greedy camera', a)
    check_masks(where + " step_versus_greedy('camera', 0)", a.unpack_masks(), view, ('camera_camera_view_mask',), plan)


def run_compensated_scene(mx, scene, where, note):
    """The random-policy flows on the plant that meets its view rims behind the first frame's kinematics and its touch rims on the
    draws of frames 0 and 1 -- frame 1 of the fused launch screens with what frame 0's range tests carried over."""
    a, b, side = mx.a, mx.b, mx.side
    plan = scene.plan
    flat = mx.flat_of(scene.state)
    side.load(RS.merged(mx.sd, scene.state))
    ref = []
    for _ in range(2):
        side.step_random()
        ref.append((side.masks(), side.batch.gather('tgt_colliding') != 0, side.batch.gather('tgt_x'), side.batch.gather('tgt_y'),
                    side.batch.gather('cam_phi'), side.batch.gather('cam_theta')))
    mx.plant(a, flat)
    a.step_random(auto_reset=False, want_masks=True)
    note('step_random', a)
    call = where + ' step_random()'
    check_masks(call, a.unpack_masks(), ref[0][0], RS.MASKS, plan)
    dev = mx.device_state(a)
    check_targets(call, dev, *ref[0][1:4], plan)
    for k, want in zip(('cam_phi', 'cam_theta'), ref[0][4:]):
        assert want.size == 0 or np.abs(dev[k].reshape(want.shape) - want).max() < POSITION_TOL, (call, k)
    for eng in (a, b):
        mx.plant(eng, flat)
    cam_r, tgt_r, sc_r = a.rollout_random(FRAMES, auto_reset=False, want_masks=True)
    note('rollout_random', a)
    call = where + ' rollout_random(%d)' % FRAMES
    check_masks(call + ' frame 0', a.unpack_masks(a._rollout['masks'][0]), ref[0][0], RS.MASKS, plan)
    check_masks(call + ' frame 1', a.unpack_masks(a._rollout['masks'][1]), ref[1][0], RS.TARGET_SIDE, plan, scene.valid_until >= 1)
    for f in range(FRAMES):
        b.step_random(auto_reset=False, want_masks=True)
        assert same(sc_r[f], b.scalars) and same(tgt_r[f], b.target_obs) and same(cam_r[f], b.camera_obs), '%s: frame %d rows / scalars differ from the single step' % (call, f)
        assert same(a._rollout['masks'][f], b.masks), '%s: frame %d masks differ from the single step' % (call, f)
        if f < 2:
            check_targets('%s frame %d (single steps of the twin)' % (call, f), mx.device_state(b), *ref[f][1:4], plan, scene.valid_until >= f)
    assert same(a.export_state(), b.export_state()), call + ': final state differs from three single steps'


@pytest.mark.parametrize('split', ['0', '1'], ids=['split0', 'split1'])
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('shape', RS.SHAPES)
def test_rims_in_every_launch_form(shape, dtype, split, oracle_lib, monkeypatch):
    monkeypatch.setenv('MATE_STEP_SPLIT', split)        # (read when an engine is created)
    mx = Matrix(shape, dtype, oracle_lib)
    scenes = RS.build_scenes(mx.sd, mx.tables, mx.cfg, RS.SEED, RS.ROUNDS[shape])
    tick = int(mx.sd['tick'][0])
    compensated = RS.build_scenes(mx.sd, mx.tables, mx.cfg, RS.SEED + 1, RS.ROUNDS[shape],
                                  random_actions=[mx.side.random_actions(tick), mx.side.random_actions(tick + 1)])
    modes = [False] + ([True] if mx.a.set_sub_wave(True) > 1 else [])
    unrecorded = []
    for mode in modes:
        for eng in (mx.a, mx.b):
            eng.set_sub_wave(mode)

        def note(call, eng):
            got = [eng.last_flow, eng.sub_wave]
            want = recorded_flow(shape, dtype, mode, split, call)
            if want is not None and got != want and (mode, call, got, want) not in unrecorded:
                unrecorded.append((mode, call, got, want))
            FLOWS_SEEN[(shape, dtype, mode, split, call)] = got

        for r, scene in enumerate(scenes):
            run_planted_scene(mx, scene, '%s %s obs sub_wave=%s MATE_STEP_SPLIT=%s plant %d' % (shape, dtype, mode, split, r), note)
        for r, scene in enumerate(compensated):
            run_compensated_scene(mx, scene, '%s %s obs sub_wave=%s MATE_STEP_SPLIT=%s compensated plant %d' % (shape, dtype, mode, split, r), note)
    for eng in (mx.a, mx.b):
        eng.close()
    assert not unrecorded, (shape, dtype, split, '(sub-wave mode, call, [last_flow, sub_wave] it ran, recorded)', unrecorded)


def test_the_matrix_ran_the_flows_recorded_for_its_calls():
    """Over the matrix above (this test reads what it noted, so it runs behind it): the set of (call, flow, environments per wave)
    seen on each recorded shape is the set tests/golden/launch_flows.json lists for these calls with set_sub_wave(False) and (True) --
    the matrix has not collapsed onto one kernel."""
    recorded_shapes = [s for s in RS.SHAPES if s in GOLDEN['flows']]
    assert len(recorded_shapes) == 5
    cells = {key[:4:3] + key[1:2] for key in FLOWS_SEEN}       # (shape, split, dtype)
    assert cells == {(s, k, d) for s in RS.SHAPES for k in ('0', '1') for d in ('f32', 'f64')}, 'run behind the whole matrix of this file (every cell notes its flows when it passes)'
    for shape in recorded_shapes:
        for dtype in ('f32', 'f64'):
            seen = {(call, tuple(v)) for (s, d, mode, split, call), v in FLOWS_SEEN.items() if s == shape and d == dtype and call in RECORDED_CALL}
            listed = set()
            for mode in (False, True):
                row = GOLDEN['flows'][shape]['%s %s plain sub_wave=%s' % (shape, dtype, mode)]
                listed |= {(call, tuple(row[CALL_ORDER.index(name)][:2])) for call, name in RECORDED_CALL.items()}
            assert seen == listed, (shape, dtype, 'seen and not listed', sorted(seen - listed), 'listed and not seen', sorted(listed - seen))
