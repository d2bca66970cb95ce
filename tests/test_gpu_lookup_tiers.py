"""GPU (-m gpu): the occlusion lookup's crowded-cell tiers, probe by probe, in every kernel form.

tests/lookup_tiers.py builds, for a natively reset batch of 22 environments, synthetic occlusion tables whose planted cells hold
exactly 5, 6, 17, 18, 37, 38, 65, 66, 257, 258, 1025 and 1026 knots (first-half, second-half and seam cells), a knot exactly on a cell
start, a repeated angle and a degree without its integer knot, and plans probes beside every selection boundary of the cell's lookup
path, at limit * (1 + 1e-6) * (1 + delta).  tests/test_lookup_tiers_cpu.py shows with the oracle alone that the plan is real.  Here
Engine.lut_write installs the tables (the obstacles stay where the reset put them: every probe is free of every circle), and
camera_target_view_mask is compared with the oracle's Camera.perceive, bit for bit per probe, through observe(), step() (f32
actions: FLOW_ACT_F32; f64 actions with a see-through tape: FLOW_ANY; MATE_STEP_SPLIT=1), step_versus_greedy('target', 0) (one launch,
MATE_POLICY_SPLIT=1, MATE_STEP_GREEDY_ROLLOUT=1), rollout_versus_greedy('target', 0, 2) (Ctx::pivots false: the quarter and narrowing
paths for the cells the per-step kernels answer from the pivot record) and, on plants pre-compensated by the Philox draw of the
targets' walk and the cameras' pose, step_random() and rollout_random(2) (row-image kernel, MATE_NO_IMAGE=1, MATE_GENERIC=1), one
and four environments per wave.  Where the cameras act on their own a probe counts in the frames in which the oracle, stepped with
the actions the device consumed, still decides it by the lookup.  Every form counts its compared probes per (tier, verdict) and must
have met every tier, G included, with both verdicts.  The fused launches are bit-identical to single steps of a twin engine.
step_greedy(), step_versus_greedy('camera', 0) and rollout_greedy(2), where the greedy targets walk, run on plants pre-compensated
by that walk itself (run_greedy_round: a fixed point over policy_actions()).  Every call asserts the [flow, environments per wave]
tests/golden/launch_flows.json records for it, or, where nothing is recorded, what engine_host.h derives.

The device builder (reset_kernels.hpp) has no lut_write in front of it: rows of tiny obstacles far from a camera with a long sight
range give it cells of 23, 32, 52 and 92 knots (T2 with pivot strides 3 and 4, T3, T4; nine obstacles give no more than 92); its
tables equal oracle.build_lut knot for knot, the probes equal the oracle through observe() and the fused rollout, and a twin engine
that took the same table through lut_write gives the same masks.

What these probes cannot tell apart, by construction of the tables: `<=` against `<` (or `>=` against `>`) in a selection of
sector_resolve.  The two differ only for a bearing EQUAL to a knot's angle, where the interpolants on both sides of the knot meet:
the limit moves by one rounding, and no bearing but a cell start (0, +-90 degrees) comes out of atan2 exactly."""
import collections
import copy

import numpy as np
import pytest
import torch

import golden_util as G
import gpu_util as U
import lookup_tiers as LT
import rim_scenes as RS
import test_gpu_rims as TR

pytestmark = pytest.mark.gpu

FLOW_ANY, FLOW_RANDOM, FLOW_ACT_F32, FLOW_GREEDY, FLOW_STEP_GREEDY = range(5)       # engine_kernels.hpp: enum Flow
SHAPES = ('MATE-4v8-9', 'MATE-8v8-9', 'MATE-4v4-9', '3v5-7')
FEW = 8                     # rounds of a form that does not run the whole plan: every plant has had probes on both sides by then
FRAMES = 2
PLAN_SEED = 7


def config_of(shape):
    cfg = copy.deepcopy(RS.config_of(shape))
    cfg['obstacle']['transmittance'] = 0.0
    return cfg


def same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


class Bench:
    """Two engines of a shape (the second one the twin that single-steps what the first one fuses) and the oracle batch, natively
    reset on the same Philox seed; the synthetic tables on all three."""

    def __init__(self, shape, dtype, O, compensated=False, max_rounds=None, switch=None):
        from mate_amd.engine import Engine
        self.shape, self.cfg = shape, config_of(shape)
        self.dtype, self.mode, self.switch = dtype, False, switch      # (row dtype, sub-wave mode, the kernel switch that is on)
        obs_dtype = torch.float64 if dtype == 'f64' else torch.float32
        self.a, self.b = (Engine(self.cfg, RS.BATCH, seed=RS.SEED, first_env_index=RS.FIRST, obs_dtype=obs_dtype) for _ in range(2))
        for eng in (self.a, self.b):
            eng.enable_policies()
            eng.reset()
        torch.cuda.synchronize()
        a = self.a
        assert a.num_obstacles > 0
        self.side = RS.OracleSide(O, shape, self.cfg)
        self.flat0 = a.export_state().cpu().numpy()
        self.sd = a.state_dict_from(self.flat0.copy())
        for k in U.STATE_KEYS:
            ref = self.side.base[k]
            assert np.array_equal(self.sd[k].reshape(ref.shape), ref), (shape, 'reset', k)
        tick = int(self.sd['tick'][0])
        self.plan = LT.build_plan(self.side.base, self.cfg, a.layout.lut_capacity, PLAN_SEED,
                                  random_actions=self.side.random_actions(tick) if compensated else None, max_rounds=max_rounds)
        for (e, c), (phis, rhos) in self.plan.tables.items():
            for eng in (self.a, self.b):
                eng.lut_write(e, c, phis, rhos)
        self.side.set_tables(LT.full_tables(self.plan.tables, [[a.lut_read(e, c) for c in range(a.num_cameras)] for e in range(RS.BATCH)]))
        n, Nc, Nt = RS.BATCH, a.num_cameras, a.num_targets
        self.no_draws = torch.zeros((n, Nc, Nt), dtype=torch.float64, device=a.device)
        self.zero_cam = {d: torch.zeros((n, Nc, 2), dtype=d, device=a.device) for d in (torch.float32, torch.float64)}
        self.zero_tgt = {d: torch.zeros((n, Nt, 2), dtype=d, device=a.device) for d in (torch.float32, torch.float64)}
        self.census = collections.defaultdict(collections.Counter)       # form -> (tier, verdict) -> compared probes
        self.worst = 0.0                                                  # largest |realised / planned - 1| of a compared probe
        self.problems = []                                                # every disagreement of the case, reported together by close()

    def flat_of(self, scene_state):
        flat = self.flat0.copy()
        for name, value in scene_state.items():
            off, shape = self.a.export_fields[name]
            k = int(np.prod(shape)) if shape else 1
            flat[:, off:off + k] = np.asarray(value, dtype=np.float64).reshape(RS.BATCH, k)
        return torch.from_numpy(flat)

    @staticmethod
    def plant(eng, flat):
        eng.import_state(flat)
        eng.observe()

    def set_sub_wave(self, mode):
        self.mode = bool(mode)
        for eng in (self.a, self.b):
            eng.set_sub_wave(mode)

    def compare(self, form, probes, bits, where):
        """The probes the oracle's current state still decides by the lookup: the device's `bits` [n, Nc, Nt] against the oracle's."""
        fields = self.side.fields()
        ref = self.side.masks()['camera_target_view_mask']
        bits = np.asarray(bits).reshape(ref.shape)
        for p in probes:
            table = self.plan.tables[(p.env, p.cam)]
            if not LT.kept(p, p.delta, fields, self.cfg, table):
                continue
            want = bool(ref[p.env, p.cam, p.tgt])
            assert want == (p.delta < 0), (where, form, p, 'the oracle itself is off the plan')
            point = (fields['tgt_x'][p.env][p.tgt], fields['tgt_y'][p.env][p.tgt])
            got_delta = LT.realised((fields['cam_x'][p.env][p.cam], fields['cam_y'][p.env][p.cam]), point, table)[1]
            self.worst = max(self.worst, abs(got_delta / p.delta - 1.0))
            tier = LT.probe_tier(p, fields, self.plan)
            if bool(bits[p.env, p.cam, p.tgt]) != want:
                self.problems.append('%s %s: environment %d camera %d target %d (%s, planted cell of %d knots, %s, tier %s, bearing %.12f, delta %+.0e) differs from the oracle' % (
                    where, form, p.env, p.cam, p.tgt, p.what, self.plan.plants[p.plant].count, self.plan.plants[p.plant].kind, tier, p.bearing, p.delta))
            self.census[form][(tier, want)] += 1

    def close(self, where):
        for eng in (self.a, self.b):
            eng.close()
        for form, count in sorted(self.census.items()):
            print('%s %s: %s' % (where, form, ' '.join('%s %d seen / %d hidden' % (t, count[(t, True)], count[(t, False)]) for t in LT.TIERS)))
        print('%s: worst realised offset off its plan by %.3g relative' % (where, self.worst))
        for line in self.problems[:40]:
            print('PROBLEM', line)
        assert not self.problems, (where, len(self.problems), self.problems[:4])
        for form, count in sorted(self.census.items()):
            missing = [(t, v) for t in LT.TIERS for v in (True, False) if not count[(t, v)]]
            assert not missing, (where, form, '(tier, verdict) never compared', missing)


def recorded(bench, name):
    """[last_flow, environments per wave] tests/golden/launch_flows.json holds for call `name` of tools/launch_matrix.py at this shape, row
    dtype and sub-wave mode (batches below the threshold, no switch), or None where it has no such column."""
    column = '%s %s plain sub_wave=%s' % (bench.shape, bench.dtype, bench.mode)
    columns = TR.GOLDEN['flows'].get(bench.shape, {})
    if bench.switch or column not in columns or name is None:
        return None
    return columns[column][TR.CALL_ORDER.index(name)][:2]


def flow_is(bench, eng, form, name, flows):
    """The call ran the recorded [flow, environments per wave]; where nothing is recorded (MATE-8v8-9, a switch, a call with a tape): one of
    `flows` (engine_host.h: folded_flow, plan_with_policies) and the mode's environments per wave."""
    got, want = [eng.last_flow, eng.sub_wave], recorded(bench, name)
    note = None
    if want is not None and got != want:
        note = '%s: [last_flow, environments per wave] %s, recorded %s' % (form, got, want)
    elif want is None and (got[0] not in flows or got[1] != (4 if bench.mode else 1)):
        note = '%s: [last_flow, environments per wave] %s, expected flow %s and %d per wave' % (form, got, flows, 4 if bench.mode else 1)
    if note and note not in bench.problems:
        bench.problems.append(note)


def versus_flows(bench):
    """step_greedy / step_versus_greedy where nothing is recorded: the two-launch form (f64 rows, MATE_POLICY_SPLIT=1) ends in the step
    kernel on caller-supplied actions; the one-launch form is step_greedy_kernel where the shape has one, else the rollout kernel
    (MATE_STEP_GREEDY_ROLLOUT=1 and four environments per wave: always)."""
    if bench.dtype == 'f64' or bench.switch == 'MATE_POLICY_SPLIT':
        return (FLOW_ACT_F32,)
    if bench.switch == 'MATE_STEP_GREEDY_ROLLOUT' or bench.mode:
        return (FLOW_GREEDY,)
    return (FLOW_STEP_GREEDY,) if bench.switch else (FLOW_GREEDY, FLOW_STEP_GREEDY)


def run_still_round(bench, state, probes, where, forms):
    """The per-step forms on one round of the plain plan: nothing moves but what the greedy cameras do."""
    a, side = bench.a, bench.side
    fields = RS.merged(bench.sd, state)
    flat = bench.flat_of(state)
    if 'observe' in forms:
        side.load(fields)
        side.update_view()
        bench.plant(a, flat)
        a.observe(tape_ct=bench.no_draws)
        flow_is(bench, a, 'observe', 'observe', (FLOW_ANY,))
        bench.compare('observe()', probes, a.unpack_masks()['camera_target_view_mask'], where)
    if 'step' in forms:
        for form, d, tape, name, flows in (('step(0, 0) f32 actions', torch.float32, None, 'step', (FLOW_ACT_F32,)),
                                          ('step(0, 0) f64 actions, tape', torch.float64, bench.no_draws, None, (FLOW_ANY,))):
            side.load(fields)
            side.step(None, None)
            bench.plant(a, flat)
            a.step(bench.zero_cam[d], bench.zero_tgt[d], tape_ct=tape, auto_reset=False)
            flow_is(bench, a, form, name, flows)
            bench.compare(form, probes, a.unpack_masks()['camera_target_view_mask'], where)
    if 'versus' in forms:
        form = "step_versus_greedy('target', 0)"
        for eng in (a, bench.b):        # (the twin too: the greedy agents keep memory from call to call, and the fused forms compare the two)
            bench.plant(eng, flat)
            eng.step_versus_greedy('target', bench.zero_tgt[torch.float32], auto_reset=False)
        flow_is(bench, a, form, 'step_versus_greedy_target', versus_flows(bench))
        cam_act = a.policy_actions()[0].cpu().numpy()
        side.load(fields)
        side.step(cam_act, None)
        bench.compare(form, probes, a.unpack_masks()['camera_target_view_mask'], where)


def run_fused_versus_round(bench, state, probes, where):
    """rollout_versus_greedy('target', 0, 2): bit-identical to two single steps of the twin, whose camera actions the oracle follows."""
    a, b, side = bench.a, bench.b, bench.side
    form = "rollout_versus_greedy('target', 0, %d)" % FRAMES
    flat = bench.flat_of(state)
    for eng in (a, b):
        bench.plant(eng, flat)
    act = bench.zero_tgt[torch.float32]
    cam_r, tgt_r, sc_r = a.rollout_versus_greedy('target', act, FRAMES, auto_reset=False, want_masks=True)
    flow_is(bench, a, form, 'rollout_versus_greedy_target', (FLOW_GREEDY,))
    side.load(RS.merged(bench.sd, state))
    for f in range(FRAMES):
        b.step_versus_greedy('target', act, auto_reset=False)
        for name, fused, single in (('scalars', sc_r[f], b.scalars), ('target rows', tgt_r[f], b.target_obs), ('camera rows', cam_r[f], b.camera_obs)):
            if not same(fused, single):
                at = tuple(int(v) for v in torch.nonzero(fused != single)[0])
                bench.problems.append('%s %s: frame %d %s differ from the single step, first at %s: %r against %r' % (where, form, f, name, at, float(fused[at]), float(single[at])))
        if not same(a._rollout['masks'][f], b.masks):
            bench.problems.append('%s %s: frame %d masks differ from the single step' % (where, form, f))
        side.step(b.policy_actions()[0].cpu().numpy(), None)
        bench.compare(form, probes, a.unpack_masks(a._rollout['masks'][f])['camera_target_view_mask'], '%s frame %d' % (where, f))
    if not same(a.export_state(), b.export_state()):
        bench.problems.append('%s %s: final state differs from single steps' % (where, form))


def run_random_round(bench, state, probes, where):
    """step_random() and rollout_random(2) on a compensated round: the probes stand on their rims behind frame 0's kinematics."""
    a, b, side = bench.a, bench.b, bench.side
    flat = bench.flat_of(state)
    fields = RS.merged(bench.sd, state)
    side.load(fields)
    side.step_random()
    bench.plant(a, flat)
    a.step_random(auto_reset=False, want_masks=True)
    flow_is(bench, a, 'step_random()', 'step_random', (FLOW_RANDOM,))
    bench.compare('step_random()', probes, a.unpack_masks()['camera_target_view_mask'], where)
    for eng in (a, b):
        bench.plant(eng, flat)
    form = 'rollout_random(%d)' % FRAMES
    cam_r, tgt_r, sc_r = a.rollout_random(FRAMES, auto_reset=False, want_masks=True)
    flow_is(bench, a, form, 'rollout_random', (FLOW_RANDOM,))
    side.load(fields)
    for f in range(FRAMES):
        b.step_random(auto_reset=False, want_masks=True)
        for name, fused, single in (('scalars', sc_r[f], b.scalars), ('target rows', tgt_r[f], b.target_obs), ('camera rows', cam_r[f], b.camera_obs)):
            if not same(fused, single):
                at = tuple(int(v) for v in torch.nonzero(fused != single)[0])
                bench.problems.append('%s %s: frame %d %s differ from the single step, first at %s: %r against %r' % (where, form, f, name, at, float(fused[at]), float(single[at])))
        if not same(a._rollout['masks'][f], b.masks):
            bench.problems.append('%s %s: frame %d masks differ from the single step' % (where, form, f))
        side.step_random()
        bench.compare(form, probes, a.unpack_masks(a._rollout['masks'][f])['camera_target_view_mask'], '%s frame %d' % (where, f))
    if not same(a.export_state(), b.export_state()):
        bench.problems.append('%s %s: final state differs from single steps' % (where, form))


GREEDY_FORMS = (('step_greedy()', 'step_greedy'), ("step_versus_greedy('camera', 0)", 'step_versus_greedy_camera'), ('rollout_greedy(%d)' % FRAMES, 'rollout_greedy'))
ITERATIONS = 6              # of the fixed point that puts a greedy target on its probe BEHIND its own step


def run_greedy_round(bench, state, probes, where):
    """The forms in which the greedy targets walk: step_greedy(), step_versus_greedy('camera', 0) and rollout_greedy(2).  A target is to
    stand on its probe behind frame 0's kinematics, so the plant is pre-compensated by the walk the device itself takes: plant, step, read
    where the oracle -- stepped with the actions the device consumed (policy_actions()) -- puts the target, move the plant by what is
    missing, again.  The walk depends only weakly on where it starts (a 20-unit shift against the distance to the goal), so the plant
    settles to 1e-9 of the probe's distance within a few rounds; every iteration is compared with the oracle in its own right, and a
    probe counts in those in which the oracle still decides it by the lookup.  Both engines take the same calls (the agents keep memory);
    the fused launch is held bit for bit to the twin's step_greedy() steps."""
    a, b, side = bench.a, bench.b, bench.side
    zero_cam = bench.zero_cam[torch.float32]
    for form, name in GREEDY_FORMS:
        if name == 'rollout_greedy' and bench.dtype == 'f64':
            continue                    # (f32 rows on the fused forms)
        start = {k: np.array(v, dtype=np.float64, copy=True) for k, v in state.items()}
        for it in range(ITERATIONS):
            flat, fields = bench.flat_of(start), RS.merged(bench.sd, start)
            for eng in (a, b):
                bench.plant(eng, flat)
            side.load(fields)
            call = '%s iteration %d' % (where, it)
            if name == 'rollout_greedy':
                cam_r, tgt_r, sc_r = a.rollout_greedy(FRAMES, auto_reset=False, want_masks=True)
                flow_is(bench, a, form, name, (FLOW_GREEDY,))
                for f in range(FRAMES):
                    b.step_greedy(auto_reset=False)
                    rows_equal(bench, '%s %s' % (call, form), f, (sc_r[f], tgt_r[f], cam_r[f], a._rollout['masks'][f]), b)
                    cam_act, tgt_act = (x.cpu().numpy() for x in b.policy_actions())
                    side.step(cam_act, tgt_act)
                    if f == 0:
                        behind = side.fields()
                    bench.compare(form, probes, a.unpack_masks(a._rollout['masks'][f])['camera_target_view_mask'], '%s frame %d' % (call, f))
                if not same(a.export_state(), b.export_state()):
                    bench.problems.append('%s %s: final state differs from single steps' % (call, form))
            else:
                for eng in (a, b):
                    if name == 'step_greedy':
                        eng.step_greedy(auto_reset=False)
                    else:
                        eng.step_versus_greedy('camera', zero_cam, auto_reset=False)
                flow_is(bench, a, form, name, versus_flows(bench))
                cam_act, tgt_act = (x.cpu().numpy() for x in a.policy_actions())
                side.step(cam_act if name == 'step_greedy' else None, tgt_act)
                behind = side.fields()
                bench.compare(form, probes, a.unpack_masks()['camera_target_view_mask'], call)
            for p in probes:            # the plant moves by what the target missed its probe by
                e, t = p.env, p.tgt
                start['tgt_x'][e, t] += state['tgt_x'][e, t] - behind['tgt_x'][e][t]
                start['tgt_y'][e, t] += state['tgt_y'][e, t] - behind['tgt_y'][e][t]


def rows_equal(bench, call, frame, fused, twin):
    for name, rows, single in zip(('scalars', 'target rows', 'camera rows', 'masks'), fused, (twin.scalars, twin.target_obs, twin.camera_obs, twin.masks)):
        if not same(rows, single):
            bench.problems.append('%s: frame %d %s differ from the single step' % (call, frame, name))


def no_episode_ends(bench):
    assert int(bench.cfg['max_episode_steps']) > FRAMES + 1


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('shape', SHAPES)
def test_tiers_in_the_per_step_forms(shape, dtype, oracle_lib):
    """observe() on the whole plan; step() with f32 actions and with f64 actions and a tape, and step_versus_greedy('target', 0), on its
    first rounds."""
    bench = Bench(shape, dtype, oracle_lib)
    where = '%s %s' % (shape, dtype)
    for r, (state, probes) in enumerate(bench.plan.rounds):
        run_still_round(bench, state, probes, '%s round %d' % (where, r), ('observe', 'step', 'versus') if r < FEW else ('observe',))
    bench.close(where)


FUSED_CASES = [(shape, False) for shape in SHAPES] + [('MATE-4v4-9', True)]       # (four environments per wave: at most four cameras and four targets)


@pytest.mark.parametrize('shape,sub_wave', FUSED_CASES)
def test_tiers_in_the_fused_forms(shape, sub_wave, oracle_lib):
    """rollout_versus_greedy('target', 0, 2) -- Ctx::pivots false -- on the whole plan, one and (the small shapes) four environments per
    wave; observe() and the per-step forms of the sub-wave kernels on the first rounds."""
    bench = Bench(shape, 'f32', oracle_lib)
    no_episode_ends(bench)
    assert not sub_wave or bench.a.set_sub_wave(True) == 4
    bench.set_sub_wave(sub_wave)
    where = '%s f32 sub_wave=%s' % (shape, sub_wave)
    for r, (state, probes) in enumerate(bench.plan.rounds):
        run_fused_versus_round(bench, state, probes, '%s round %d' % (where, r))
        if sub_wave and r < FEW:
            run_still_round(bench, state, probes, '%s round %d' % (where, r), ('observe', 'step', 'versus'))
    bench.close(where)


@pytest.mark.parametrize('shape,sub_wave', FUSED_CASES)
def test_tiers_under_the_random_policy(shape, sub_wave, oracle_lib):
    """step_random() and rollout_random(2) on plants pre-compensated by the Philox draw of the targets' walk and the cameras' pose."""
    bench = Bench(shape, 'f32', oracle_lib, compensated=True)
    no_episode_ends(bench)
    assert not sub_wave or bench.a.set_sub_wave(True) == 4
    bench.set_sub_wave(sub_wave)
    where = '%s f32 sub_wave=%s compensated' % (shape, sub_wave)
    for r, (state, probes) in enumerate(bench.plan.rounds):
        run_random_round(bench, state, probes, '%s round %d' % (where, r))
    bench.close(where)


@pytest.mark.parametrize('shape,sub_wave,dtype', [(s, w, 'f32') for s, w in FUSED_CASES] + [(s, False, 'f64') for s in SHAPES])
def test_tiers_with_the_greedy_targets(shape, sub_wave, dtype, oracle_lib):
    """step_greedy(), step_versus_greedy('camera', 0) and (f32 rows) rollout_greedy(2) on the first rounds of the plan, the plant
    pre-compensated by the greedy targets' own walk."""
    bench = Bench(shape, dtype, oracle_lib, max_rounds=FEW)
    no_episode_ends(bench)
    assert not sub_wave or bench.a.set_sub_wave(True) == 4
    bench.set_sub_wave(sub_wave)
    where = '%s %s sub_wave=%s' % (shape, dtype, sub_wave)
    for r, (state, probes) in enumerate(bench.plan.rounds):
        run_greedy_round(bench, state, probes, '%s round %d' % (where, r))
    bench.close(where)


@pytest.mark.parametrize('switch', ['MATE_STEP_SPLIT', 'MATE_POLICY_SPLIT', 'MATE_STEP_GREEDY_ROLLOUT', 'MATE_NO_IMAGE', 'MATE_GENERIC'])
def test_tiers_under_the_kernel_switches(switch, oracle_lib, monkeypatch):
    """MATE-4v8-9 with one switch on (read when an engine is created): the forms the switch changes.  MATE_POLICY_SPLIT and
    MATE_STEP_GREEDY_ROLLOUT show in the flow of step_versus_greedy (the step kernel, the rollout kernel; step_greedy_kernel without them)
    and MATE_GENERIC in Engine.specialised; the library reports nothing about MATE_STEP_SPLIT and MATE_NO_IMAGE, so for every switch the
    name is held to the list in include/mate_engine.h."""
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'mate_engine.h')) as fh:
        assert ' *   %s=' % switch in fh.read()
    assert TR.GOLDEN['flows']['MATE-4v8-9']['MATE-4v8-9 f32 plain sub_wave=False'][TR.CALL_ORDER.index('step_versus_greedy_target')][0] == FLOW_STEP_GREEDY
    monkeypatch.setenv(switch, '1')
    fused = switch in ('MATE_NO_IMAGE', 'MATE_GENERIC')
    where = 'MATE-4v8-9 f32 %s=1' % switch
    if fused:
        bench = Bench('MATE-4v8-9', 'f32', oracle_lib, compensated=True, max_rounds=2 * FEW, switch=switch)
        assert bench.a.specialised == (switch != 'MATE_GENERIC')
        for r, (state, probes) in enumerate(bench.plan.rounds):
            run_random_round(bench, state, probes, '%s round %d' % (where, r))
        bench.close(where)
    bench = Bench('MATE-4v8-9', 'f32', oracle_lib, max_rounds=2 * FEW, switch=switch)
    for r, (state, probes) in enumerate(bench.plan.rounds):
        if fused:
            run_fused_versus_round(bench, state, probes, '%s round %d' % (where, r))
        else:
            run_still_round(bench, state, probes, '%s round %d' % (where, r), ('observe', 'step', 'versus'))
    bench.close(where)


# ------------------------------------------------------------------ the device builder
def _natural_engine(obstacles, n=1):
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-1v1-9.yaml', camera={'max_sight_range': LT.NATURAL_RMAX}, obstacle={'transmittance': 0.0})
    eng = Engine(cfg, n, seed=1, obs_dtype=torch.float32)
    eng.enable_policies()
    eng.reset()
    assert (eng.num_cameras, eng.num_targets, eng.num_obstacles) == (1, 1, 9)
    return cfg, eng


@pytest.mark.parametrize('scene', sorted(LT.NATURAL_SCENES))
def test_device_builder_on_crowded_cells(scene, oracle_lib):
    """Rows of tiny obstacles seen from far away: the device builder's table equals oracle.build_lut knot for knot, the probes of its
    fullest cell equal the oracle through observe() (pivots true) and rollout_versus_greedy (pivots false), and a twin engine that took
    the same table through lut_write -- the host builder's records -- gives the same masks."""
    O = oracle_lib
    obstacles, tier = LT.NATURAL_SCENES[scene]
    want_phis, want_rhos = O.build_lut(LT.NATURAL_CAMERA, LT.NATURAL_RMAX, obstacles)
    n = LT.NATURAL_N
    cfg, eng = _natural_engine(obstacles, n)
    _, twin = _natural_engine(obstacles, n)
    cam = np.full((n, 1), LT.NATURAL_CAMERA[0]), np.full((n, 1), LT.NATURAL_CAMERA[1])
    theta = LT.NATURAL_THETA
    sight = float(np.sqrt(30.0 * LT.NATURAL_RMAX ** 2 / theta))
    state = {'cam_x': cam[0], 'cam_y': cam[1], 'cam_phi': np.full((n, 1), LT.natural_phi(want_phis)), 'cam_theta': np.full((n, 1), theta),
             'obs_x': np.broadcast_to(obstacles[:, 0], (n, 9)), 'obs_y': np.broadcast_to(obstacles[:, 1], (n, 9)),
             'obs_radius': np.broadcast_to(obstacles[:, 2], (n, 9))}
    for e_ in (eng, twin):
        e_.load_state_dict(state)
    eng.rebuild_luts()
    torch.cuda.synchronize()
    phis, rhos = eng.lut_read(0, 0)
    assert len(phis) == len(want_phis) and np.abs(phis - want_phis).max() < 1e-9, (scene, len(phis), len(want_phis))
    G.assert_only_tangent_flips(phis, rhos, want_rhos, LT.NATURAL_CAMERA, LT.NATURAL_RMAX, obstacles, 1e-7, scene)
    points = LT.natural_probes(phis, rhos)          # (on the device's own knots: a tangent-ray coin flip moves a knot, not the lookup)
    state.update(tgt_x=np.array([p[0][0] for p in points]).reshape(n, 1), tgt_y=np.array([p[0][1] for p in points]).reshape(n, 1))
    counts = LT.cell_counts(phis)[1]
    assert LT.tier_of(int(counts.max())) == tier, (scene, int(counts.max()))
    for e in range(n):
        twin.lut_write(e, 0, phis, rhos)
    census = collections.Counter()
    want = np.array([O.camera_perceive(LT.NATURAL_CAMERA, state['cam_phi'][0, 0], theta, sight, p[0], 0.0, 0.0, phis, rhos) for p in points])
    assert np.array_equal(want, np.array([p[1] < 0 for p in points])), scene
    zero = torch.zeros((n, 1, 2), dtype=torch.float32, device=eng.device)
    no_draws = torch.zeros((n, 1, 1), dtype=torch.float64, device=eng.device)
    for form in ('observe()', 'rollout_versus_greedy'):
        got = []
        for e_ in (eng, twin):
            e_.load_state_dict({'tgt_x': state['tgt_x'], 'tgt_y': state['tgt_y'], 'cam_phi': state['cam_phi'], 'cam_theta': state['cam_theta']})
            if form == 'observe()':
                e_.observe(tape_ct=no_draws)
                assert e_.last_flow == FLOW_ANY
                got.append(e_.unpack_masks()['camera_target_view_mask'][:, 0, 0])
            else:       # the caller holds the target still, the greedy camera acts
                e_.observe()
                e_.rollout_versus_greedy('target', zero, 1, auto_reset=False, want_masks=True)
                assert e_.last_flow == FLOW_GREEDY
                got.append(e_.unpack_masks(e_._rollout['masks'][0])['camera_target_view_mask'][:, 0, 0])
        assert np.array_equal(got[0], got[1]), (scene, form, 'device builder and lut_write differ on probes', np.flatnonzero(got[0] != got[1])[:8])
        if form == 'observe()':
            keep = np.ones(n, dtype=bool)
        else:           # the greedy camera has moved: the probes its new pose still decides by the lookup
            sd = eng.state_dict()
            s2 = np.sqrt(30.0 * LT.NATURAL_RMAX ** 2 / sd['cam_theta'][:, 0])
            keep = np.array([LT.decided_by_lookup(LT.NATURAL_CAMERA, sd['cam_phi'][e, 0], sd['cam_theta'][e, 0], s2[e], points[e][0]) for e in range(n)])
        bad = np.flatnonzero((got[0] != want) & keep)
        assert not len(bad), (scene, form, [(points[i], bool(got[0][i])) for i in bad[:6]])
        for i in np.flatnonzero(keep):
            census[(form, bool(want[i]))] += 1
    print('%s (fullest cell %d knots, %s): %s' % (scene, int(counts.max()), tier, dict(census)))
    assert all(census[(f, v)] >= 4 for f in ('observe()', 'rollout_versus_greedy') for v in (True, False)), census
    eng.close()
    twin.close()
