"""The plan of tests/lookup_tiers.py is real: with the oracle alone, on the shapes, batch and seed tests/test_gpu_lookup_tiers.py runs,
the tier rule restates the header's constants, every planted cell holds exactly its planned count, every (tier, threshold count, cell
kind) holds at least four kept probes of each verdict, the oracle's Camera.perceive gives every kept probe the verdict its side says,
at most 2 % of the planned probes are dropped, and the natural-geometry scenes of the device-builder test reach their tiers."""
import collections
import copy

import numpy as np
import pytest

import lookup_tiers as LT
import rim_scenes as RS

SHAPES = ('MATE-4v8-9', 'MATE-8v8-9', 'MATE-4v4-9', '3v5-7')
MIN_COUNT = 4
MAX_DROPPED = 0.02


def test_tier_rule_restates_the_header():
    import os
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, '..', 'mate_amd', 'csrc', 'engine_kernels.hpp')) as fh:
        text = fh.read()
    assert int(re.search(r'constexpr int kDegSlots = (\d+);', text).group(1)) == LT.K_DEG_SLOTS == 5
    assert 'constexpr int kPivotKnots = 9 * (kDegSlots - 1) + 1;' in text and LT.K_PIVOT_KNOTS == 37
    assert 'constexpr int kQuarterKnots = 4 * (kDegSlots - 1) + 1;' in text and LT.K_QUARTER_KNOTS == 17
    assert 'while (count > kQuarterKnots && count <= 4 * 256 + 1)' in text
    assert 'pivot_stride(int count) { return (count - 1 + 8) / 9; }' in text
    tops = {'T0': 5, 'T1': 17, 'T2': 37, 'T3': 4 * 16 + 1, 'T4': 4 * 64 + 1, 'T5': 4 * 256 + 1}
    for tier, top in tops.items():
        assert LT.tier_of(top) == tier and LT.tier_of(top + 1) == LT.TIERS[LT.TIERS.index(tier) + 1]
    assert LT.tier_of(2) == 'T0' and LT.tier_of(2027) == 'T6'
    # one narrowing level takes 65 knots to at most 17, two take 257, three 1025 (sector_resolve: q = (count + 2) / 4, then q + 1 knots)
    for count, levels in ((38, 1), (65, 1), (66, 2), (257, 2), (258, 3), (1025, 3)):
        k, n = count, 0
        while k > LT.K_QUARTER_KNOTS:
            k, n = (k + 2) // 4 + 1, n + 1
        assert n == levels, (count, n)
    assert [LT.pivot_stride(c) for c in (6, 10, 11, 37)] == [1, 1, 2, 4]


@pytest.mark.parametrize('compensated', [False, True], ids=['plain', 'compensated'])
@pytest.mark.parametrize('shape', SHAPES)
def test_the_planted_cells_and_probes_are_where_the_plan_says(shape, compensated, oracle_lib):
    cfg = copy.deepcopy(RS.config_of(shape))
    cfg['obstacle']['transmittance'] = 0.0
    side = RS.OracleSide(oracle_lib, shape, cfg)
    kmax = 360 + 185 * side.No + 2
    plan = LT.build_plan(side.base, cfg, kmax, 7, random_actions=side.random_actions(int(side.base['tick'][0])) if compensated else None)
    fallback = side.tables()
    assert all(len(t[0]) <= kmax for t in plan.tables.values())
    for phis, rhos in plan.tables.values():
        assert phis[0] == -180.0 and phis[-1] == 180.0 and rhos[-1] == rhos[0] and np.all(np.diff(phis) >= 0.0)
    planted = collections.Counter()
    for plant in plan.plants:
        phis, rhos = plan.tables[(plant.env, plant.cam)]
        sight = float(np.sqrt(cfg['camera']['min_viewing_angle'] * cfg['camera']['max_sight_range'] ** 2 / plan.poses[(plant.env, plant.cam)][1]))
        assert rhos.min() >= 0.2 * sight and rhos.max() <= 0.85 * sight, (shape, plant)
        if plant.kind != 'missing':
            assert int(LT.cell_counts(phis)[1][plant.cell]) == plant.count, (shape, plant)
        if plant.kind in LT.CELL_KINDS:       # a bracket off by one knot moves the limit by at least 1e-3 relative
            k0 = plant.first
            step = np.abs(np.diff(rhos[k0:k0 + plant.count])) / rhos[k0:k0 + plant.count - 1]
            assert step.min() >= 1e-3, (shape, plant, float(step.min()))
            assert np.all(np.diff(phis) > 0.0) and plant.tier == LT.tier_of(plant.count)
            planted[(plant.count, plant.kind)] += 1
    assert all(planted[(c, k)] >= 1 for c in LT.THRESHOLD_COUNTS for k in LT.CELL_KINDS), planted
    assert {p.kind for p in plan.plants} >= {'halfstart', 'repeat', 'missing'}
    side.set_tables(LT.full_tables(plan.tables, fallback))
    census, tiers = collections.Counter(), collections.Counter()
    worst = 0.0
    for state, probes in plan.rounds:
        fields = RS.merged(side.base, state)
        side.load(fields)
        if compensated:
            side.step_random()
        else:
            side.update_view()
        now = side.fields()
        seen = side.masks()['camera_target_view_mask']
        for p in probes:
            table = plan.tables[(p.env, p.cam)]
            assert LT.kept(p, p.delta, now, cfg, table), (shape, p)
            got = LT.realised((now['cam_x'][p.env][p.cam], now['cam_y'][p.env][p.cam]), (now['tgt_x'][p.env][p.tgt], now['tgt_y'][p.env][p.tgt]), table)[1]
            worst = max(worst, abs(got / p.delta - 1.0))
            verdict = bool(seen[p.env, p.cam, p.tgt])
            assert verdict == (p.delta < 0), (shape, p, got)
            plant = plan.plants[p.plant]
            census[(plant.tier, plant.count, plant.kind, verdict)] += 1
            tiers[(LT.probe_tier(p, now, plan), verdict)] += 1
    low = {k: v for k, v in census.items() if v < MIN_COUNT}
    assert not low, (shape, low)
    want = {(LT.tier_of(c), c, k, v) for c in LT.THRESHOLD_COUNTS for k in LT.CELL_KINDS for v in (True, False)}
    assert want <= set(census), (shape, want - set(census))
    assert all(tiers[(t, v)] >= MIN_COUNT for t in LT.TIERS for v in (True, False)), tiers
    kept_probes = sum(len(p) for _, p in plan.rounds)
    assert kept_probes + plan.dropped == plan.planned and plan.dropped <= MAX_DROPPED * plan.planned, (shape, plan.dropped, plan.planned)
    print('%s %s: %d probes in %d rounds, %d of %d planned dropped, worst realised offset off its plan by %.3g relative; by tier: %s' % (
        shape, 'compensated' if compensated else 'plain', kept_probes, len(plan.rounds), plan.dropped, plan.planned, worst,
        ' '.join('%s %d/%d' % (t, tiers[(t, True)], tiers[(t, False)]) for t in LT.TIERS)))


@pytest.mark.parametrize('scene', sorted(LT.NATURAL_SCENES))
def test_natural_scenes_reach_their_tiers(scene, oracle_lib):
    obstacles, tier = LT.NATURAL_SCENES[scene]
    assert obstacles.shape == (9, 3)
    phis, rhos = oracle_lib.build_lut(LT.NATURAL_CAMERA, LT.NATURAL_RMAX, obstacles)
    assert len(phis) <= 360 + 185 * 9 + 2
    counts = LT.cell_counts(phis)[1]
    assert LT.tier_of(int(counts.max())) == tier, (scene, int(counts.max()))
    points = LT.natural_probes(phis, rhos)
    sight = float(np.sqrt(30.0 * LT.NATURAL_RMAX ** 2 / LT.NATURAL_THETA))
    verdicts = collections.Counter()
    for point, delta in points:
        assert LT.decided_by_lookup(LT.NATURAL_CAMERA, LT.natural_phi(phis), LT.NATURAL_THETA, sight, point)
        seen = oracle_lib.camera_perceive(LT.NATURAL_CAMERA, LT.natural_phi(phis), LT.NATURAL_THETA, sight, point, 0.0, 0.0, phis, rhos)
        assert seen == (delta < 0), (scene, point, delta)
        verdicts[seen] += 1
    assert min(verdicts[True], verdicts[False]) >= 16, verdicts
    print('%s: %d knots, fullest cell %d (%s), probes %s' % (scene, len(phis), int(counts.max()), tier, dict(verdicts)))
