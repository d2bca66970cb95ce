"""The plan of tests/rim_scenes.py is real: with the oracle alone, on the shapes, batch, seed and rounds tests/test_gpu_rims.py runs,
every planted probe stands where the plan says -- its realised offset from the rim, in exact rational arithmetic on the f64 state
(f64 for the two rims that go through atan2 and the occlusion table), is within a factor 2 of the planned one -- every rim kind,
ladder step and side occurs at least four times, the f32 band of the range test is populated inside and just outside both edges, both
verdicts occur on every rim kind, and the touch probes do what their side says."""
import collections

import numpy as np
import pytest

import rim_scenes as RS

MIN_COUNT = 4


def _within_factor_2(realised, planned):
    return abs(realised) < 1e-15 if planned == 0.0 else 0.5 < realised / planned < 2.0


def _coverage(plan, what):
    count = collections.Counter((RS.family(p.kind), p.rung, p.frame) for p in plan)
    low = {k: v for k, v in count.items() if v < MIN_COUNT}
    assert not low, (what, low)
    return {p.kind for p in plan}


@pytest.mark.parametrize('shape', RS.SHAPES)
def test_the_planted_rims_are_where_the_plan_says(shape, oracle_lib):
    side = RS.OracleSide(oracle_lib, shape)
    cfg, tables = side.cfg, side.tables()
    scenes = RS.build_scenes(side.base, tables, cfg, RS.SEED, RS.ROUNDS[shape])
    plan = [p for s in scenes for p in s.plan]
    kinds = _coverage(plan, shape)
    want = {'sense_target', 'sense_camera', 'cc_edge', 'cc_sight', 'ct_edge', 'ct_sight', 'touch_camera'}
    want |= {'sense_obstacle', 'ct_lookup', 'touch_obstacle'} if side.No else set()
    assert kinds == want, (shape, kinds ^ want)
    for fam in {RS.family(k) for k in kinds}:      # every ladder step of the rim, both sides, both frames
        ladder = {'sense': len(RS.range_ladder(500.0)), 'cc_edge': 8, 'ct_edge': 8, 'cc_sight': 11, 'ct_sight': 11, 'ct_lookup': 6,
                  'touch': 2 * len(RS.TOUCH_RUNGS)}[fam]
        assert len({(p.rung, p.frame) for p in plan if RS.family(p.kind) == fam}) == ladder, (shape, fam)
    verdicts = collections.defaultdict(set)
    in_band, outside = 0, collections.Counter()
    for scene in scenes:
        fields = RS.merged(side.base, scene.state)
        side.load(fields)
        side.update_view()
        masks = side.masks()
        for p in scene.plan:
            if p.kind.startswith('touch'):
                continue
            got = RS.realised_offset(p, fields, cfg, tables)
            assert _within_factor_2(got, p.delta), (shape, RS.describe([p]), got)
            seen = RS.probe_verdict(p, masks)
            verdicts[p.kind].add(seen)
            if p.rung != '0':
                assert seen == (p.side < 0), (shape, RS.describe([p]), got)
            if p.kind.startswith('sense'):
                a, b, lim = RS.probe_geometry(p, fields, cfg)
                off2 = float(RS.exact_offset(a[0], a[1], b[0], b[1], lim)) * float(sum(lim)) ** 2      # on the squared distance
                band = RS.f32_band(sum(lim))
                in_band += abs(off2) < band
                outside[np.sign(off2)] += band < abs(off2) < 1.2 * band
        # touch probes: the oracle walks the action; at the probe's frame the target stands on the rim and does what its side says
        positions = [np.stack([fields['tgt_x'], fields['tgt_y']], axis=-1)]
        for frame in range(2):
            now = dict(fields, tgt_x=positions[-1][..., 0], tgt_y=positions[-1][..., 1])
            for p in scene.plan:
                if p.kind.startswith('touch') and p.frame == frame:
                    got = RS.realised_offset(p, now, cfg, tables)
                    assert _within_factor_2(got, p.delta), (shape, RS.describe([p]), got)
            side.step(None, scene.actions)
            positions.append(np.stack([side.batch.gather('tgt_x'), side.batch.gather('tgt_y')], axis=-1))
            colliding = side.batch.gather('tgt_colliding') != 0
            for p in scene.plan:
                if p.kind.startswith('touch') and p.frame == frame:
                    e, t = p.env, p.pair[0]
                    a, b, lim = RS.probe_geometry(p, now, cfg)
                    step, reach = float(lim[0]), float(sum(lim))
                    dest = positions[-2][e, t] + RS.clamped(scene.actions[e, t], step)
                    short = float(np.hypot(*(dest - positions[-1][e, t])))
                    what = RS.touch_expectation(p, reach)
                    verdicts[p.kind].add(what != 'miss')
                    if what == 'miss':
                        assert short < 1e-12 and not colliding[e, t], (shape, RS.describe([p]), short)
                    else:
                        assert 0.5 < short / (reach * abs(p.delta)) < 2.0, (shape, RS.describe([p]), short)
                        assert colliding[e, t] == (what == 'collide'), (shape, RS.describe([p]), short)
    sense = sum(p.kind.startswith('sense') for p in plan)
    assert 3 * in_band >= sense and outside[-1.0] >= MIN_COUNT and outside[1.0] >= MIN_COUNT, (shape, sense, in_band, dict(outside))
    assert all(v == {False, True} for v in verdicts.values()) and set(verdicts) == kinds, (shape, dict(verdicts))


@pytest.mark.parametrize('shape', RS.SHAPES)
def test_the_compensated_plant_meets_its_rims_after_the_random_step(shape, oracle_lib):
    """The plant of the random-policy flows is pose - action: after the oracle's own step on the Philox draws the probes stand within
    a factor 2 of the planned offsets (1e-9 and up), and the oracle's verdict is the side's."""
    side = RS.OracleSide(oracle_lib, shape)
    cfg, tables = side.cfg, side.tables()
    draws = [side.random_actions(0), side.random_actions(1)]
    scenes = RS.build_scenes(side.base, tables, cfg, RS.SEED + 1, RS.ROUNDS[shape], random_actions=draws)
    plan = [p for s in scenes for p in s.plan]
    assert all(abs(p.delta) >= 0.999e-9 for p in plan)
    kinds = _coverage(plan, shape)
    want = {'sense_target', 'sense_camera', 'cc_edge', 'cc_sight', 'ct_edge', 'ct_sight', 'touch_camera'}
    assert kinds == want | ({'sense_obstacle', 'touch_obstacle'} if side.No else set()), (shape, kinds)
    verdicts = collections.defaultdict(set)
    step_size = float(cfg['target']['step_size'])
    for scene in scenes:
        side.load(RS.merged(side.base, scene.state))
        for frame in range(2):
            before = side.fields()
            side.step_random()
            after, masks = side.fields(), side.masks()
            colliding = side.batch.gather('tgt_colliding') != 0
            for p in scene.plan:
                if p.frame != frame:
                    continue
                if not p.kind.startswith('touch'):      # the view rims hold behind the first step, whose walk there was clean
                    got = RS.realised_offset(p, after, cfg, tables)
                    assert _within_factor_2(got, p.delta), (shape, RS.describe([p]), got)
                    seen = RS.probe_verdict(p, masks)
                    assert seen == (p.side < 0), (shape, RS.describe([p]), got)
                    assert p.kind[:2] == 'cc' or not colliding[p.env, p.pair[0 if p.kind.startswith('sense') else 1]]
                    verdicts[p.kind].add(seen)
                    continue
                e, t = p.env, p.pair[0]
                walk = RS.clamped(draws[frame][1][e][t].astype(np.float64), step_size / before['tgt_capacity'][e][t])
                walked = float(np.hypot(*walk))
                got = RS.realised_offset(p, before, cfg, tables, walked)
                assert _within_factor_2(got, p.delta), (shape, RS.describe([p]), got)
                a, b, lim = RS.probe_geometry(p, before, cfg, walked)
                reach = float(sum(lim))
                short = float(np.hypot(before['tgt_x'][e][t] + walk[0] - after['tgt_x'][e][t], before['tgt_y'][e][t] + walk[1] - after['tgt_y'][e][t]))
                what = RS.touch_expectation(p, reach)
                verdicts[p.kind].add(what != 'miss')
                if what == 'miss':
                    assert short < 1e-12 and not colliding[e, t], (shape, RS.describe([p]), short)
                else:
                    assert 0.5 < short / (reach * abs(p.delta)) < 2.0, (shape, RS.describe([p]), short)
                    assert colliding[e, t] == (what == 'collide'), (shape, RS.describe([p]), short)
    assert all(v == {False, True} for v in verdicts.values()) and set(verdicts) == kinds, (shape, dict(verdicts))
