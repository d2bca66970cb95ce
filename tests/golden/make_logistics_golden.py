#!/usr/bin/env python3
"""Generator of tests/golden/kat_logistics.npz: the reference's own MultiAgentTracking._assign_goals (environment.py:1271-1324) on the
planted warehouse states of tests/logistics_scenes.py, one environment's worth per row.

A row is what _assign_goals meets on frame 0 or 1 of a planted scene of MATE-4v8-9 or MATE-2v4-0: the target locations behind the
walk and the tracked bits of that view (both from the oracle's step: they are INPUTS here), and the goals, goal bits, empty bits,
freights, bounties, counters, remaining / awaiting / delivered cargoes in front of the rule.  The fields are put into a reference
environment of the row's scenario, `np_random` is replaced by a tape (choice(a) = a[min(int(u * len(a)), len(a) - 1)] off the row's
uniforms, one per target, as the oracle and the device take them), the reference's method is called, and every output is stored:
both rewards, goals, goal bits, empty bits, freights, bounties, the counters, remaining, awaiting, delivered, target_dones and
target_warehouse_distances.  Arrays and names only: data, no program text.  Rows of 4-target scenes are padded to 8 targets
(`num_targets` tells); environments whose episode has ended and the scenes' untouched 'none' environments are left out.

    MATE_REFERENCE=<checkout of XuehaiPan/mate> python tests/golden/make_logistics_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG  # noqa: E402,F401  (puts the shim and the reference on sys.path, imports gym and mate)
import mate  # noqa: E402

import logistics_scenes as LS  # noqa: E402
import rim_scenes as RS  # noqa: E402

KAT_SHAPES = ('MATE-4v8-9', 'MATE-2v4-0')
KAT_ROUNDS = 2
MAXT = 8
PER_TARGET = ('tgt_goals', 'freights', 'bounties', 'target_steps', 'tracked_steps')
IN_KEYS = ('tgt_x', 'tgt_y', 'tgt_capacity', 'tracked_bits', 'goal_u') + LS.LOGISTICS_KEYS[:10]
OUT_KEYS = LS.LOGISTICS_KEYS[:10] + ('target_dones', 'target_warehouse_distances', 'reward', 'delayed_reward')


class Tape:
    """np_random of _assign_goals: the t-th target's pick comes off the t-th uniform (t: the caller's loop variable)."""

    def __init__(self, uniforms):
        self.uniforms = uniforms

    def choice(self, a):
        a = np.asarray(a)
        t = sys._getframe(1).f_locals['t']
        return a[LS.pick_index(float(self.uniforms[t]), len(a))]


def reference_row(env, row):
    """_assign_goals of the reference on one row's inputs -> the row's outputs."""
    Nt = env.num_targets
    for t, target in enumerate(env.targets):
        target.location = np.array([row['tgt_x'][t], row['tgt_y'][t]], dtype=np.float64)
        target.goal_bits[:] = row['tgt_goal_bits'][t]
        target.empty_bits[:] = row['tgt_empty_bits'][t] != 0
    env.target_capacities = row['tgt_capacity'][:Nt].astype(np.int64)
    env.target_goals = row['tgt_goals'][:Nt].astype(np.int64)
    env.target_goal_bits = row['tgt_goal_bits'][:Nt].astype(np.int64)
    env.freights = row['freights'][:Nt].astype(np.int64)
    env.bounties = row['bounties'][:Nt].astype(np.int64)
    env.target_steps = row['target_steps'][:Nt].astype(np.int64)
    env.tracked_steps = row['tracked_steps'][:Nt].astype(np.int64)
    env.tracked_bits = row['tracked_bits'][:Nt] != 0
    env.remaining_cargoes = row['remaining_cargoes'].reshape(4, 4).astype(np.int64)
    env.awaiting_cargo_counts = row['awaiting_cargo_counts'].astype(np.int64)
    env.num_delivered_cargoes = int(row['num_delivered_cargoes'])
    env._np_random = Tape(row['goal_u'])
    reward, delayed = env._assign_goals()
    pad = lambda a, fill=0: np.concatenate([np.asarray(a, dtype=np.float64), np.full((MAXT - Nt,) + np.shape(a)[1:], fill, dtype=np.float64)])  # noqa: E731
    return {'tgt_goals': pad(env.target_goals, -1), 'tgt_goal_bits': pad(env.target_goal_bits), 'freights': pad(env.freights), 'bounties': pad(env.bounties),
            'tgt_empty_bits': pad(np.stack([target.empty_bits for target in env.targets])),
            'target_steps': pad(env.target_steps), 'tracked_steps': pad(env.tracked_steps),
            'remaining_cargoes': np.asarray(env.remaining_cargoes, dtype=np.float64).reshape(-1), 'awaiting_cargo_counts': np.asarray(env.awaiting_cargo_counts, dtype=np.float64),
            'num_delivered_cargoes': np.float64(env.num_delivered_cargoes), 'target_dones': pad(env.target_dones),
            'target_warehouse_distances': pad(env.target_warehouse_distances), 'reward': np.float64(reward), 'delayed_reward': np.float64(delayed)}


def rows_of(shape, O):
    """The inputs of every row of a shape, off the oracle's walk through the planted scenes (tests/logistics_scenes.py)."""
    side = RS.OracleSide(O, shape)
    Nt = side.Nt
    scenes = LS.build_scenes(side.base, side.tables(), side.cfg, LS.SEED, LS.ROUNDS[shape])[:KAT_ROUNDS]
    pad = lambda a, fill=0: np.concatenate([np.asarray(a, dtype=np.float64).reshape((Nt,) + np.shape(a)[1:]), np.full((MAXT - Nt,) + np.shape(a)[1:], fill, dtype=np.float64)])  # noqa: E731
    rows = []
    for r, scene in enumerate(scenes):
        side.load(RS.merged(side.base, scene.state))
        live = np.ones(LS.BATCH, dtype=bool)
        for frame in range(2):
            before = side.fields()
            LS.oracle_step(side, scene.actions, scene.goal_u, live=live)
            after = side.fields()
            tracked = side.batch.gather('tracked_bits')
            for e in np.flatnonzero(live):
                if LS.scene_kind(e) == 'none':
                    continue
                row = {'tgt_x': pad(after['tgt_x'][e]), 'tgt_y': pad(after['tgt_y'][e]), 'tgt_capacity': pad(before['tgt_capacity'][e], 1),
                       'tracked_bits': pad(tracked[e]), 'goal_u': pad(scene.goal_u[e], 0.5)}
                for k in LS.LOGISTICS_KEYS[:10]:
                    v = np.asarray(before[k][e], dtype=np.float64)
                    if k in ('tgt_goal_bits', 'tgt_empty_bits'):
                        row[k] = pad(v.reshape(Nt, 4))
                    elif k in PER_TARGET:
                        row[k] = pad(v, -1 if k == 'tgt_goals' else 0)
                    else:
                        row[k] = v.reshape(-1) if v.ndim else v
                row['where'] = (shape, r, frame, int(e))
                row['probes'] = '%s round %d frame %d environment %d: %s' % (shape, r, frame, e, '; '.join(LS.describe(LS.probes_at(scene.plan, e))))
                rows.append(row)
            live &= side.batch.gather('done') == 0
    return rows, side.cfg


def main():
    from oracle import oracle as O
    O.build()
    out = {'shapes': np.asarray(KAT_SHAPES)}
    ins, outs, where, probes, counts = [], [], [], [], []
    for s, shape in enumerate(KAT_SHAPES):
        rows, cfg = rows_of(shape, O)
        env = mate.make('MultiAgentTracking-v0', config=shape + '.yaml')
        env.seed(0)
        env.reset()
        out.setdefault('freight_scale', np.float64(env.freight_scale))
        out.setdefault('bounty_scale', np.float64(env.bounty_scale))
        assert out['freight_scale'] == env.freight_scale and out['bounty_scale'] == env.bounty_scale
        for row in rows:
            ins.append(row)
            outs.append(reference_row(env, row))
            where.append((s,) + row['where'][1:])
            probes.append(row['probes'])
            counts.append(env.num_targets)
    for k in IN_KEYS:
        out['in/' + k] = np.stack([row[k] for row in ins])
    for k in OUT_KEYS:
        out['out/' + k] = np.stack([row[k] for row in outs])
    out['where'] = np.asarray(where, dtype=np.int64)            # (index into `shapes`, round, frame, environment)
    out['num_targets'] = np.asarray(counts, dtype=np.int64)
    out['probes'] = np.asarray(probes)
    path = os.path.join(HERE, 'kat_logistics.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    changed = sum(bool((out['out/' + k] != out['in/' + k]).any()) for k in LS.LOGISTICS_KEYS[:10])
    print('kat_logistics.npz: %d rows, %d of 10 state fields change somewhere, %d rows deliver, %.0f KiB'
          % (len(ins), changed, int((out['out/num_delivered_cargoes'] > out['in/num_delivered_cargoes']).sum()), size / 1024))
    assert changed >= 9 and size < 256 * 1024, (changed, size)


if __name__ == '__main__':
    main()
