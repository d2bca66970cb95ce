"""The plan of tests/logistics_scenes.py is real, shown with the oracle alone on the shapes, batch, seed and rounds
tests/test_gpu_logistics.py runs: (a) the oracle's assign_goals reproduces every row the reference's own _assign_goals left in
tests/golden/kat_logistics.npz; (b) every probe lands, bit for bit, on its planned point and on its planned side of the warehouse
box (exact rational arithmetic), does there what the plan expects (picks up, delivers, passes, loses to a lower index, ends the
episode), every catalogue entry occurs at least twice, on both frames, and none was left out; (c) the census that is the reason for
these scenes: the random policy puts no target in a warehouse."""
import collections
import os

import numpy as np
import pytest

import logistics_scenes as LS
import rim_scenes as RS

MIN_COUNT = 2
KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kat_logistics.npz')
KAT_INT = ('tgt_goals', 'tgt_goal_bits', 'tgt_empty_bits', 'freights', 'bounties', 'target_steps', 'tracked_steps', 'remaining_cargoes',
           'awaiting_cargo_counts', 'num_delivered_cargoes', 'target_dones')
KAT_DISTANCE_TOL = 1e-12      # relative: two f64 roots of the same sum of squares


def test_the_oracle_reproduces_the_reference_on_every_recorded_row(oracle_lib):
    kat = np.load(KAT)
    n, Nt = kat['in/tgt_x'].shape
    env = oracle_lib.OracleEnv(0, Nt, 0)
    env.set('freight_scale', float(kat['freight_scale'])); env.set('bounty_scale', float(kat['bounty_scale']))
    delivered_rows = 0
    for i in range(n):
        nt = int(kat['num_targets'][i])
        for k in ('tgt_x', 'tgt_y', 'tgt_capacity', 'tracked_bits') + KAT_INT[:10]:
            env.set(k, kat['in/' + k][i])
        reward, delayed = env.assign_goals(kat['in/goal_u'][i])
        assert reward == kat['out/reward'][i] and delayed == kat['out/delayed_reward'][i], (i, str(kat['probes'][i]), reward, delayed)
        for k in KAT_INT:
            got, want = env.get(k), kat['out/' + k][i]
            assert np.array_equal(np.asarray(got).reshape(want.shape), want), (i, k, str(kat['probes'][i]))
        got, want = env.get('target_warehouse_distances')[:nt], kat['out/target_warehouse_distances'][i][:nt]
        assert np.all(np.abs(got - want) <= KAT_DISTANCE_TOL * want), (i, str(kat['probes'][i]))
        delivered_rows += kat['out/num_delivered_cargoes'][i] > kat['in/num_delivered_cargoes'][i]
    assert n >= 100 and delivered_rows >= 20 and (kat['out/reward'] != kat['out/delayed_reward']).any()


def _check_probe(p, before, after, side, scene, shape, taped=True):
    """What the plan expects of probe p, on the oracle's state before and behind the probe's frame."""
    e, t, w = p.env, p.target, p.warehouse
    what = (shape, LS.describe([p]))
    x, y = after['tgt_x'][e][t], after['tgt_y'][e][t]
    assert (x, y) == p.landing, what + ((x, y),)
    assert LS.exact_side(x, y) == p.side and (p.side > 0 or LS.warehouse_at(x, y) == w), what
    if p.rung == 'clip':
        assert after['tgt_colliding'][e][t] and max(abs(x), abs(y)) == RS.TERRAIN and p.side < 0, what
    tracked = bool(side.envs[e].get('tracked_bits')[t])
    if p.tracked is not None:
        assert tracked == p.tracked, what
    goal0, goal1 = int(before['tgt_goals'][e][t]), int(after['tgt_goals'][e][t])
    delivered = after['num_delivered_cargoes'][e] - before['num_delivered_cargoes'][e]
    empty = after['tgt_empty_bits'][e].reshape(-1, 4)[t][w]
    row_empty = not after['remaining_cargoes'][e].reshape(4, 4)[w].any()
    if p.expect == 'outside':
        for k in ('tgt_goals', 'tgt_goal_bits', 'tgt_empty_bits', 'freights'):
            assert np.array_equal(np.asarray(before[k][e]).reshape(side.Nt, -1)[t], np.asarray(after[k][e]).reshape(side.Nt, -1)[t]), what + (k,)
        return tracked
    if p.kind != 'shared':               # (there the row empties under a later arrival: the bit is the row's state at the visit)
        assert empty == row_empty, what
    if p.expect == 'pickup':
        assert goal0 == -1 and goal1 >= 0 and goal1 != w and after['freights'][e][t] > 0 and after['target_steps'][e][t] == 1, what
        if p.kind == 'pick' and taped:
            assert goal1 == p.detail, what
    elif p.expect == 'lose':
        assert goal0 == -1 and goal1 == -1 and empty and after['freights'][e][t] == 0, what
    elif p.expect == 'pass':
        assert goal0 == goal1 >= 0 and goal1 != w and after['freights'][e][t] == before['freights'][e][t], what
        assert after['target_steps'][e][t] == before['target_steps'][e][t] + 1, what
    elif p.expect == 'deliver':
        assert goal0 == w and delivered >= before['tgt_goal_bits'][e].reshape(-1, 4)[t][w] > 0 and after['target_steps'][e][t] == 1, what
    return tracked


def _run_scene(side, scene, shape, random_policy=False):
    """Both probe frames of a scene on the oracle; -> {probe: tracked}, {environment: frame at which it ended}."""
    side.load(RS.merged(side.base, scene.state))
    seen, ended = {}, {}
    live = np.ones(LS.BATCH, dtype=bool)
    for frame in range(LS.FRAMES):
        before = side.fields()
        if random_policy:
            side.step_random()
        else:
            LS.oracle_step(side, scene.actions, scene.goal_u, live=live)
        after = side.fields()
        done = side.batch.gather('done') != 0
        for p in scene.plan:
            if p.frame == frame:
                assert live[p.env], (shape, LS.describe([p]), 'the episode ended before the probe')
                seen[p] = _check_probe(p, before, after, side, scene, shape, taped=not random_policy)
        for e in np.flatnonzero(done & live):
            ended[int(e)] = frame
        if not random_policy:
            live &= ~done
    return seen, ended


def _end_expectations(scene, ended, cfg, shape):
    for p in scene.plan:
        if p.kind != 'end':
            continue
        what = (shape, LS.describe([p]), ended.get(p.env))
        if p.rung in ('last', 'last_limit-1', 'last_limit', 'open_limit'):
            assert ended.get(p.env) == p.frame, what            # by cargo, by the time limit, by both
        elif p.rung == 'open_limit-1':
            assert ended.get(p.env) == p.frame + 1, what        # one step later, by the time limit
        else:
            assert p.env not in ended, what
    for e, frame in ended.items():
        assert LS.scene_kind(e) == 'end', (shape, e, frame)


@pytest.mark.parametrize('shape', LS.SHAPES)
def test_the_planted_logistics_are_what_the_plan_says(shape, oracle_lib):
    side = RS.OracleSide(oracle_lib, shape)
    cfg, tables = side.cfg, side.tables()
    scenes = LS.build_scenes(side.base, tables, cfg, LS.SEED, LS.ROUNDS[shape])
    plan = [p for s in scenes for p in s.plan]
    # nothing left out: every environment of a kind holds the probes its kind plants
    per_env = collections.Counter((r, p.env) for r, s in enumerate(scenes) for p in s.plan)
    for r in range(len(scenes)):
        for e in range(LS.BATCH):
            kind = LS.scene_kind(e)
            want = {'none': 0, 'rim': side.Nt, 'carry': min(side.Nt, 4), 'delivery': side.Nt, 'shared': 2, 'pick': min(side.Nt, 4), 'end': 1}[kind]
            assert per_env[(r, e)] >= want and (kind != 'none' or per_env[(r, e)] == 0), (shape, r, e, kind, per_env[(r, e)], want)
    count = collections.Counter((ent, p.frame) for p in plan for ent in LS.entries(p))
    two_ton = any(2 in np.asarray(side.base['tgt_capacity'][e]) for e in range(LS.BATCH) if LS.scene_kind(e) == 'delivery')
    for ent in LS.catalogue(side.Nt):
        if ent == ('delivery', 'weight 2') and not two_ton:
            continue
        assert count[(ent, 0)] >= 1 and count[(ent, 1)] >= 1 and count[(ent, 0)] + count[(ent, 1)] >= MIN_COUNT, (shape, ent, count[(ent, 0)], count[(ent, 1)])
    assert {p.side for p in plan if p.kind == 'rim'} == {-1, 1}
    tracked = collections.Counter()
    for scene in scenes:
        seen, ended = _run_scene(side, scene, shape)
        assert set(seen) == set(scene.plan)
        _end_expectations(scene, ended, cfg, shape)
        for p, tr in seen.items():
            tracked[(p.kind, tr)] += 1
            if p.kind == 'delivery':
                tracked[(p.rung.split('bounty ')[1], tr)] += 1
    if side.Nc:      # deliveries under a camera's eye and out of it, and the bounty that decays to 0 on the step of its delivery
        assert tracked[('delivery', True)] >= MIN_COUNT and tracked[('delivery', False)] >= MIN_COUNT and tracked[('one', True)] >= 1, (shape, dict(tracked))


@pytest.mark.parametrize('shape', LS.SHAPES)
def test_the_compensated_plant_lands_on_the_random_policys_own_draws(shape, oracle_lib):
    """position = landing - the draws of OracleSide.random_actions: behind the oracle's own random step(s) every probe stands on its
    planned point, bit for bit, and does what the plan expects -- with the goal pick off the Philox stream both sides share."""
    side = RS.OracleSide(oracle_lib, shape)
    cfg, tables = side.cfg, side.tables()
    draws = [side.random_actions(0), side.random_actions(1)]
    scenes = LS.build_scenes(side.base, tables, cfg, LS.SEED + 1, LS.ROUNDS[shape], draws=draws)
    plan = [p for s in scenes for p in s.plan]
    kinds = collections.Counter((p.kind, p.frame) for p in plan)
    for kind in ('rim', 'carry', 'delivery', 'pick', 'end'):
        assert kinds[(kind, 0)] >= MIN_COUNT, (shape, dict(kinds))
    if side.Nt >= 8:
        assert all(kinds[(kind, 1)] >= 1 for kind in ('rim', 'delivery', 'end')) and kinds[('shared', 0)] >= 1, (shape, dict(kinds))
    assert {p.side for p in plan if p.kind == 'rim'} == {-1, 1}
    for scene in scenes:
        assert not scene.actions.any()
        seen, ended = _run_scene(side, scene, shape, random_policy=True)
        assert set(seen) == set(scene.plan)


def test_the_random_policy_reaches_no_warehouse(oracle_lib):
    """Why the scenes are planted: 64 natively reset MATE-4v8-9 environments x 50 random steps, and no target ever stands inside a
    warehouse box, no goal changes, nothing is delivered -- every random-policy test of the suite steps with an empty warehouse mask."""
    import gpu_util as U
    cfg = RS.config_of('MATE-4v8-9')
    batch = oracle_lib.OracleBatch(U.oracle_proto_from_config(cfg, oracle_lib), 64, seed=31, first_env_index=7)
    batch.reset(threads=4)
    goals = batch.gather('tgt_goals')
    for _ in range(50):
        batch.step(auto_reset=False, threads=4)
        x, y = batch.gather('tgt_x'), batch.gather('tgt_y')
        sup = np.maximum(np.abs(np.abs(x) - LS.CENTRE), np.abs(np.abs(y) - LS.CENTRE))
        assert not (sup <= LS.RADIUS).any()
        assert np.array_equal(batch.gather('tgt_goals'), goals) and not batch.gather('num_delivered_cargoes').any()
