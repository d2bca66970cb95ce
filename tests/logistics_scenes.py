"""Goal logistics on planted warehouse scenes: shared by tests/golden/make_logistics_golden.py (the reference's own _assign_goals on
the planted states -> kat_logistics.npz), tests/test_logistics_scenes_cpu.py (the oracle alone: is the plan real?) and
tests/test_gpu_logistics.py (every launch form against the oracle).  Pure NumPy, built as tests/rim_scenes.py is.

_assign_goals (environment.py:1271-1324) is the one order-dependent rule of the step: a target inside a warehouse box (Chebyshev
distance <= 75 from (+-925, +-925)) delivers, picks up from the warehouse's row of the shared `remaining_cargoes` in index order,
learns that the warehouse is empty; the episode ends with the last awaited cargo.  No random-policy trajectory reaches a warehouse
(tests/test_logistics_scenes_cpu.py restates the census), so the scenes PLANT targets one or two steps in front of a landing point
and everything they carry, on natively reset batches of rim_scenes.BATCH environments:

  env % 7   kind      what is planted
  0         rim       landings on a ladder around the inner edges |x| = 850, |y| = 850 (the edge, +-1 and +-2 ulps, 1e-12 ... 1e-5
                      relative), the inner corner and one ulp outside it in one coordinate, a point inside the box but further than 75
                      from the centre, a point inside in x and outside in y, the outer edge through the terrain clip; the arriving
                      target unloaded, loaded for this warehouse, loaded for another
  1         none      nothing (sub-wave kernels step it in one wave with environments that have a target inside)
  2         carry     the three loads against an empty and a stocked warehouse row: what happens to the empty bits
  3         delivery  weight 1 / 2, bounty full / part-decayed / 1 / 0, a reload or an empty row behind the delivery, cameras aimed at
                      the warehouse or away from it
  4         shared    two or three unloaded targets arrive on one frame where the row holds cargo for fewer; capacity against remaining
                      1 and 5; arrivals in different warehouses
  5         pick      rows with 1, 2, 3 positive entries, zeros between; the goal tape at j/k, one ulp below, 0 and nextafter(1, 0)
  6         end       the last awaited cargo; episode_step at the time limit and one short of it, with and without that delivery; no
                      bounty anywhere; the first delivery of an episode

Every probe holds on frame 0 or on frame 1 (planted one more step out).  The walk is an unclamped f32 action, so the landing is
exact on both sides: start + action (+ action) == landing in f64, and x - 925 is exact, so every rung is decided beyond rounding
(exact_side).  `draws`: the random policy's own actions replace the chosen ones (position = landing - draws), on targets whose draws
are not clamped.
"""
import collections
from fractions import Fraction

import numpy as np

import rim_scenes as RS

CENTRE, RADIUS, EDGE = 925.0, 75.0, 850.0
SIGNS = np.array([[1.0, 1.0], [-1.0, 1.0], [-1.0, -1.0], [1.0, -1.0]])       # constants.py:70-72
WAREHOUSES = SIGNS * CENTRE
KINDS = ('rim', 'none', 'carry', 'delivery', 'shared', 'pick', 'end')
FRAMES = 3
SHAPES, BATCH, SEED, FIRST = RS.SHAPES, RS.BATCH, RS.SEED, RS.FIRST
# plants per engine: enough for every catalogue entry to occur twice and on both frames (tests/test_logistics_scenes_cpu.py counts)
ROUNDS = {'MATE-2v4-0': 7, 'MATE-4v4-9': 7, 'MATE-4v8-0': 5, 'MATE-4v8-9': 5, '3v5-7': 6, 'MATE-4v2-9': 11, 'MATE-8v8-9': 5}
LOGISTICS_KEYS = ('tgt_goals', 'tgt_goal_bits', 'tgt_empty_bits', 'freights', 'bounties', 'target_steps', 'tracked_steps', 'remaining_cargoes',
                  'awaiting_cargo_counts', 'num_delivered_cargoes', 'episode_step', 'episode_reward', 'delayed_episode_reward')
PLANTED_KEYS = ('tgt_x', 'tgt_y', 'cam_phi', 'cam_theta') + LOGISTICS_KEYS

# env; kind; target; warehouse; rung: the catalogue entry; frame: the step at which it holds; side: -1 inside a warehouse, +1 outside;
# expect: 'pickup' | 'deliver' | 'pass' (loaded for another warehouse) | 'lose' (nothing left for it) | 'outside'; detail: entry-specific
# (the goal a taped pick must choose, the bounty planted, ...); tracked: True / False where the plant decides it, None where it does not;
# landing: the f64 point the target stands on behind that step
Probe = collections.namedtuple('Probe', 'env kind target warehouse rung frame side expect detail tracked landing')
Scene = collections.namedtuple('Scene', 'state actions goal_u plan')


def scene_kind(env):
    return KINDS[env % len(KINDS)]


def _ulps(v, k):
    for _ in range(abs(k)):
        v = float(np.nextafter(v, np.inf if k > 0 else -np.inf))
    return v


def warehouse_at(x, y):
    """The warehouse that holds (x, y), or -1: the reference's `supremum <= 75` in exact rational arithmetic on the f64 values."""
    for w, (wx, wy) in enumerate(WAREHOUSES):
        if max(abs(Fraction(float(x)) - int(wx)), abs(Fraction(float(y)) - int(wy))) <= int(RADIUS):
            return w
    return -1


def exact_side(x, y):
    return -1 if warehouse_at(x, y) >= 0 else 1


# the ladder on an inner edge: (name, |coordinate| on the edge's axis); inside iff >= 850
EDGE_RUNGS = [('edge', EDGE)] + [('ulp%+d' % k, _ulps(EDGE, k)) for k in (-2, -1, 1, 2)] + [('%+.0e' % d, EDGE * (1.0 + d)) for d in RS.RIM_DELTAS]
# ... and the points that are no edge rung: (name, (|x|, |y|) before the axes are swapped)
POINT_RUNGS = [('corner', (EDGE, EDGE)), ('corner_out', (_ulps(EDGE, -1), EDGE)), ('euclid', (856.0, 856.0)), ('in_x_out_y', (900.0, 845.0)), ('clip', None)]
RIM_RUNGS = [r[0] for r in EDGE_RUNGS + POINT_RUNGS]
CARRIES = ('unloaded', 'here', 'elsewhere')
BOUNTIES = ('full', 'part', 'one', 'zero')
SHARED = ('two_for_one', 'three_for_two', 'plenty', 'split')
END = ('last', 'last_limit-1', 'last_limit', 'open_limit-1', 'open_limit', 'first_delivery', 'no_bounty')


def pick_tape(k):
    """The goal-tape values planted against a row with k positive entries: [(name, u, index chosen)]."""
    out = [('u=0', 0.0, 0), ('u=1-', float(np.nextafter(1.0, 0.0)), k - 1)]
    for j in range(1, k):
        out += [('u=%d/%d' % (j, k), j / k, j), ('u=%d/%d-' % (j, k), float(np.nextafter(j / k, 0.0)), j - 1)]
    return out


PICKS = [('k%d %s' % (k, name), k, u, j) for k in (1, 2, 3) for name, u, j in pick_tape(k)]


def pick_index(u, k):
    """np_random.choice(candidates) off a uniform, as the oracle and the device take it: min(int(u * k), k - 1)."""
    return min(int(u * k), k - 1)


class _Plant:
    """One environment while it is planted: the logistics fields, the walks, the camera poses."""

    def __init__(self, base, e, cfg, tables, rng, draws):
        self.e, self.cfg, self.rng, self.draws = e, cfg, rng, draws
        self.env = RS._Env(base, e, cfg, tables)
        self.Nt, self.Nc = len(self.env.tgt), len(self.env.cam)
        self.cap = np.asarray(base['tgt_capacity'][e], dtype=np.int64).reshape(-1)
        self.f = {k: np.array(base[k][e], dtype=np.float64, copy=True) for k in PLANTED_KEYS}
        self.f['tgt_goal_bits'] = self.f['tgt_goal_bits'].reshape(self.Nt, 4)
        self.f['tgt_empty_bits'] = self.f['tgt_empty_bits'].reshape(self.Nt, 4)
        self.f['remaining_cargoes'] = self.f['remaining_cargoes'].reshape(4, 4)
        self.actions = np.zeros((self.Nt, 2))
        self.goal_u = np.full(self.Nt, 0.5)
        self.used = set()                   # targets that walk
        self.landings = {}                  # target -> (landing, warehouse, frame)
        tgt = cfg['target']
        self.freight_scale = float(np.ceil(2000.0 / tgt['step_size']))
        self.bounty_scale = float(np.ceil(self.freight_scale * max(0.0, cfg['bounty_factor'])))
        # a running episode, so that no counter is compared at zero
        self.f['episode_step'] = np.float64(100 + e)
        self.f['num_delivered_cargoes'] = np.float64(3)
        self.f['episode_reward'] = np.float64(3 * self.freight_scale + 140.0 - e)
        self.f['delayed_episode_reward'] = np.float64(3 * self.freight_scale + 95.0)

    # ---- what a target carries
    def unload(self, t):
        f = self.f
        f['tgt_goals'][t] = -1; f['tgt_goal_bits'][t] = 0; f['freights'][t] = 0; f['bounties'][t] = 0
        f['target_steps'][t] = 4 + t; f['tracked_steps'][t] = t % 3

    def load(self, t, goal, weight, bounty='part'):
        f = self.f
        total = weight * self.bounty_scale
        b = {'full': total, 'part': total - 37.0 - t, 'one': 1.0, 'zero': 0.0}[bounty]
        f['tgt_goals'][t] = goal; f['tgt_goal_bits'][t] = 0; f['tgt_goal_bits'][t, goal] = weight
        f['freights'][t] = weight * self.freight_scale; f['bounties'][t] = b
        f['tracked_steps'][t] = total - b + (5 if b == 0.0 else 0)
        f['target_steps'][t] = f['tracked_steps'][t] + 11 + t
        return b

    def stock(self, w, row):
        assert row[w] == 0                  # the reset never makes cargo for its own warehouse
        self.f['remaining_cargoes'][w] = row

    def other_goal(self, w, shift=0):
        return [g for g in range(4) if g != w][shift % 3]

    # ---- the walk
    def usable(self, t, frame):
        """Under the random policy: the draws of the frames up to the probe's are not clamped (the landing is then exact)."""
        if t in self.used:
            return False
        if self.draws is None:
            return True
        return all(np.hypot(*self.draws[k][1][self.e][t].astype(np.float64)) <= self.env.step[t] * (1.0 - 1e-6) for k in range(frame + 1))

    def _clear(self, a, b, margin=1.0):
        env = self.env
        if not len(env.circles):
            return True
        ab = b - a
        s = np.clip(((env.circles - a) @ ab) / max(float(ab @ ab), 1e-300), 0.0, 1.0)
        return bool(np.all(np.hypot(*(env.circles - (a + s[:, None] * ab)).T) - env.circle_r > margin))

    def walk(self, t, w, landing, frame, axis=0, clip=False):
        """Target t stands on `landing` behind frame `frame`: plants its start and (without draws) its action.  False where the walk
        meets a circle, is clamped, or enters a warehouse early."""
        landing = np.asarray(landing, dtype=np.float64)
        step = float(self.env.step[t])
        if not self.usable(t, frame):
            return False
        if self.draws is None:
            a = np.zeros(2)
            a[axis] = SIGNS[w][axis] * 0.85 * step
            a[1 - axis] = self.rng.choice([-1.0, 1.0]) * 0.1 * step
            if clip:                        # diagonal: the other coordinate crosses the inner edge on the step that runs into the terrain's edge
                a[:] = SIGNS[w] * 0.6 * step
            a = a.astype(np.float32).astype(np.float64)
            acts = [a] * FRAMES
        else:
            if clip:
                return False
            acts = [self.draws[k][1][self.e][t].astype(np.float64) for k in range(frame + 1)]
        if clip:                            # the first coordinate runs into the terrain's edge and is cut there
            start = landing - (frame + 1) * acts[0]
            start[axis] = SIGNS[w][axis] * RS.TERRAIN - (frame + 0.5) * acts[0][axis]
        else:
            start = landing - sum(acts[:frame + 1])
        for _settle in range(6):
            path = [start]
            for k in range(frame + 1):
                path.append(np.clip(path[-1] + acts[k], -RS.TERRAIN, RS.TERRAIN))
            if np.array_equal(path[-1], landing):
                break
            start = start + (landing - path[-1])
        else:
            return False
        if any(exact_side(*p) < 0 for p in path[:-1]):
            return False
        for k in range(frame + 1, len(acts)):
            path.append(np.clip(path[-1] + acts[k], -RS.TERRAIN, RS.TERRAIN))
        if not all(self._clear(p, q) for p, q in zip(path[:-1], path[1:])):
            return False
        self.f['tgt_x'][t], self.f['tgt_y'][t] = start
        if self.draws is None:
            self.actions[t] = acts[0]
        self.used.add(t)
        self.landings[t] = (landing, w, frame)
        return True

    def deep(self, w, axis=0):
        """A landing well inside warehouse w, near the inner edge of `axis` (within one step of a capacity-2 target of the outside)."""
        p = np.zeros(2)
        p[axis] = EDGE + self.rng.uniform(1.0, 4.0)
        p[1 - axis] = CENTRE + self.rng.uniform(-40.0, 40.0)
        return p * SIGNS[w]

    def arrive(self, t, w, frame):
        """Target t walks to a deep landing in w or, where that walk is not clean, in the next warehouse that takes it: -> w or None."""
        for shift in range(4):
            for axis in (0, 1):
                w2 = (w + shift) % 4
                if self.walk(t, w2, self.deep(w2, axis), frame, axis):
                    return w2
        return None

    def free_targets(self, frame):
        return [t for t in range(self.Nt) if self.usable(t, frame)]

    # ---- cameras
    def aim(self, want, used_warehouses):
        """Every camera looks at the warehouse `want` (None: at one no probe uses, or across the terrain's middle edge)."""
        env = self.env
        spare = [w for w in range(4) if w not in used_warehouses]
        for c in range(self.Nc):
            if want is not None:
                at = WAREHOUSES[want]
            elif spare:
                at = WAREHOUSES[spare[0]]
            else:
                continue
            rel = at - env.cam[c]
            env.phi[c] = float(np.rad2deg(np.arctan2(rel[1], rel[0])))
            env.theta[c] = env.theta_min
        self.f['cam_phi'], self.f['cam_theta'] = env.phi.copy(), env.theta.copy()

    def tracked(self, point):
        """True: some camera surely sees `point` (in its sector and sight by a margin, nearer than its occlusion table);
        False: surely none does; None: too close to call."""
        if self.draws is not None:
            return None
        env, verdicts = self.env, []
        for c in range(self.Nc):
            rel = np.asarray(point) - env.cam[c]
            d, bearing = float(np.hypot(*rel)), float(np.rad2deg(np.arctan2(rel[1], rel[0])))
            off = abs(RS._norm_angle(bearing - env.phi[c])) - env.theta[c] / 2.0
            sight = env.cam_sight(c)
            if off > 0.5 or d > 1.01 * sight:
                verdicts.append(False)
            elif off < -0.5 and d < 0.99 * sight and d < 0.99 * RS.lut_at(env.tables[c], bearing):
                verdicts.append(True)
            else:
                verdicts.append(None)
        return True if True in verdicts else (None if None in verdicts else False)

    def finish(self):
        f = self.f
        f['awaiting_cargo_counts'] = f['remaining_cargoes'].sum(axis=0) + f['tgt_goal_bits'].sum(axis=0)


def build_scenes(state, tables, cfg, seed, rounds, draws=None):
    """`rounds` planted copies of a natively reset `state` ([n, ...] arrays over gpu_util.STATE_KEYS).  Returns [Scene]: the planted
    fields, the target team's joint action [n, Nt, 2] (f32 values, none clamped; zero with `draws`), the goal tape [n, Nt] and the
    plan [Probe].  `draws` = [(camera actions, target actions) of the random policy at the next tick, the one after]."""
    rng = np.random.RandomState(seed)
    n = len(state['tgt_x'])
    Nt = np.shape(state['tgt_x'])[1]
    count = collections.Counter()
    scenes = []
    max_steps = int(cfg['max_episode_steps'])
    for rnd in range(rounds):
        out = {k: np.array(state[k], dtype=np.float64, copy=True) for k in PLANTED_KEYS}
        out['tgt_goal_bits'] = out['tgt_goal_bits'].reshape(n, Nt, 4)
        out['tgt_empty_bits'] = out['tgt_empty_bits'].reshape(n, Nt, 4)
        out['remaining_cargoes'] = out['remaining_cargoes'].reshape(n, 4, 4)
        actions, goal_u, plan = np.zeros((n, Nt, 2)), np.full((n, Nt), 0.5), []
        for e in range(n):
            kind = scene_kind(e)
            P = _Plant(state, e, cfg, tables[e], rng, draws)
            probes = []                     # (target, warehouse, rung, frame, expect, detail)
            want_tracked = None

            if kind == 'rim':
                for w in range(4):
                    P.stock(w, [0 if g == w else 3 for g in range(4)])
                for t in range(Nt):
                    idx = count['rim']
                    rungs = RIM_RUNGS if draws is None else RIM_RUNGS[:-1]         # (no draw is known to run into the terrain's edge)
                    name = rungs[idx % len(rungs)]
                    frame, axis = (idx // len(rungs)) % 2, (idx // (2 * len(rungs))) % 2
                    if draws is not None:       # few targets have unclamped draws: both frames from the first lap on
                        frame = idx % 2 if P.usable(t, idx % 2) else 0
                        name = rungs[(idx // 2 + (idx % 2 + idx // len(rungs)) * (len(rungs) // 2)) % len(rungs)]
                    carry = CARRIES[idx % 3]
                    for shift in range(4):
                        w = (idx + shift) % 4
                        other = CENTRE + rng.uniform(-40.0, 40.0)
                        if name == 'clip':
                            p = np.zeros(2); p[axis], p[1 - axis] = RS.TERRAIN, EDGE + 0.25 * P.env.step[t]
                        elif name in dict(EDGE_RUNGS):
                            p = np.zeros(2); p[axis], p[1 - axis] = dict(EDGE_RUNGS)[name], other
                        else:
                            p = np.array(dict(POINT_RUNGS)[name])[[axis, 1 - axis]] if axis else np.array(dict(POINT_RUNGS)[name])
                        if P.walk(t, w, p * SIGNS[w], frame, axis, clip=name == 'clip'):
                            break
                    else:
                        continue
                    count['rim'] += 1
                    side = exact_side(*P.landings[t][0])
                    if carry == 'unloaded':
                        P.unload(t)
                    else:
                        P.load(t, w if carry == 'here' else P.other_goal(w, idx), 1 if carry == 'here' else int(P.cap[t]))
                    P.f['tgt_empty_bits'][t] = [(t + g) % 2 for g in range(4)]
                    expect = 'outside' if side > 0 else {'unloaded': 'pickup', 'here': 'deliver', 'elsewhere': 'pass'}[carry]
                    probes.append((t, w, name, frame, expect, carry))

            elif kind == 'carry':
                for t in range(Nt):
                    idx = count['carry']
                    carry, stocked = CARRIES[idx % 3], (idx // 3) % 2
                    frame = (idx // 6) % 2
                    taken = {p[1] for p in probes}
                    w = next((w for w in ((idx + s) % 4 for s in range(4)) if w not in taken), None)
                    if w is None or not P.usable(t, frame):
                        continue
                    w = P.arrive(t, w, frame)
                    if w is None or w in taken:
                        if w is not None:
                            P.used.discard(t); P.f['tgt_x'][t], P.f['tgt_y'][t] = state['tgt_x'][e][t], state['tgt_y'][e][t]; P.actions[t] = 0
                        continue
                    count['carry'] += 1
                    P.stock(w, [0 if g == w or not stocked else 2 for g in range(4)])
                    if carry == 'unloaded':
                        P.unload(t)
                    else:
                        P.load(t, w if carry == 'here' else P.other_goal(w, idx), 1)
                    P.f['tgt_empty_bits'][t] = 0
                    P.f['tgt_empty_bits'][t, w] = stocked          # (the wrong way round: the visit corrects it)
                    expect = {'unloaded': 'pickup' if stocked else 'lose', 'here': 'deliver', 'elsewhere': 'pass'}[carry]
                    probes.append((t, w, '%s %s' % (carry, 'stocked' if stocked else 'empty'), frame, expect, stocked))

            elif kind == 'delivery':
                want_tracked = (count['delivery_env'] // 2 + count['delivery_env']) % 2 == 0       # (against the rotation of the bounties)
                count['delivery_env'] += 1
                for t in range(Nt):
                    idx = count['delivery']
                    bounty, reload = BOUNTIES[idx % 4], (idx // 4) % 2
                    frame = (idx // 8) % 2
                    weight = 2 if P.cap[t] == 2 and (idx // 16) % 2 == 0 else 1
                    w0 = probes[0][1] if probes else idx % 4           # one warehouse per environment: the cameras look at it or away
                    if not P.usable(t, frame) or not P.walk(t, w0, P.deep(w0, idx % 2), frame, idx % 2):
                        if probes or P.arrive(t, w0, frame) is None:
                            continue
                    w = P.landings[t][1]
                    count['delivery'] += 1
                    planted = P.load(t, w, weight, bounty)
                    if not probes:
                        P.stock(w, [0 if g == w or not reload else 4 for g in range(4)])
                    probes.append((t, w, 'weight %d bounty %s' % (weight, bounty), frame, 'deliver', planted))

            elif kind == 'shared':
                idx = count['shared']
                variant, frame = SHARED[idx % 4], (idx // 4) % 2
                free = P.free_targets(frame)
                arrivals = min(3 if variant == 'three_for_two' else 2, len(free))
                if arrivals >= 2:
                    chosen = sorted(int(t) for t in rng.choice(free, arrivals, replace=False))
                    order = list(rng.permutation(chosen))          # (placed in any order: the index decides, not the placement)
                    w = idx % 4
                    placed = {}
                    for i, t in enumerate(order):
                        target_w = (w + 1 + i) % 4 if variant == 'split' else (placed[order[0]] if placed else w)
                        if placed and variant != 'split':
                            got = target_w if any(P.walk(t, target_w, P.deep(target_w, ax), frame, ax) for ax in (0, 1)) else None
                        else:
                            got = P.arrive(t, target_w, frame)
                        if got is not None:
                            placed[t] = got
                            P.unload(t)
                            P.f['tgt_empty_bits'][t] = 0
                    if len(placed) >= 2 and (variant == 'split') == (len(set(placed.values())) == len(placed)):
                        count['shared'] += 1
                        first = min(placed)
                        for w2 in set(placed.values()):
                            g1, g2 = P.other_goal(w2, idx), P.other_goal(w2, idx + 1)
                            row = [0, 0, 0, 0]
                            if variant == 'plenty':
                                row[g1] = 5
                            elif variant == 'three_for_two' and len(placed) == 3:
                                row[g1] = row[g2] = 1
                            else:
                                row[g1] = 1
                            P.stock(w2, row)
                        stock = {w2: int(sum(P.f['remaining_cargoes'][w2] > 0)) if variant != 'plenty' else 9 for w2 in set(placed.values())}
                        for t in sorted(placed):
                            w2 = placed[t]
                            wins = stock[w2] > 0
                            stock[w2] -= 1
                            rung = '%s x%d cap%d' % (variant, len(placed), int(P.cap[first]))
                            probes.append((t, w2, rung, frame, 'pickup' if wins else 'lose', 'two_for_one' if variant == 'three_for_two' and len(placed) < 3 else variant))

            elif kind == 'pick':
                for t in range(min(Nt, 4)):
                    idx = count['pick']
                    name, k, u, j = PICKS[idx % len(PICKS)]
                    frame = (idx // len(PICKS)) % 2
                    taken = {p[1] for p in probes}
                    w = next((w for w in ((idx + s) % 4 for s in range(4)) if w not in taken), None)
                    if w is None or not P.usable(t, frame):
                        continue
                    w = P.arrive(t, w, frame)
                    if w is None or w in taken:
                        if w is not None:
                            P.used.discard(t); P.f['tgt_x'][t], P.f['tgt_y'][t] = state['tgt_x'][e][t], state['tgt_y'][e][t]; P.actions[t] = 0
                        continue
                    count['pick'] += 1
                    cands = [g for g in range(4) if g != w]
                    chosen = {1: [cands[idx % 3]], 2: [cands[0], cands[2]], 3: cands}[k]
                    P.stock(w, [2 + g if g in chosen else 0 for g in range(4)])
                    P.unload(t)
                    P.goal_u[t] = u
                    assert pick_index(u, k) == j
                    probes.append((t, w, name, frame, 'pickup', chosen[j]))

            elif kind == 'end':
                idx = count['end']
                variant, frame = END[idx % len(END)], (idx // len(END)) % 2
                free = P.free_targets(frame)
                if free:
                    t = free[idx % len(free)]
                    w = P.arrive(t, idx % 4, frame)
                    if w is not None:
                        count['end'] += 1
                        f = P.f
                        if variant.startswith('last') or variant == 'no_bounty':
                            f['remaining_cargoes'][:] = 0
                        if variant.startswith('last'):
                            for t2 in range(Nt):
                                P.unload(t2)
                        if variant == 'no_bounty':
                            f['tracked_steps'] += f['bounties'] + 2
                            f['bounties'][:] = 0
                        else:
                            P.stock(w, [0, 0, 0, 0])
                        weight = int(P.cap[t]) if idx % 2 else 1
                        P.load(t, w, weight, 'zero' if variant == 'no_bounty' else 'part')
                        if variant.startswith('open'):
                            w2 = (w + 1) % 4
                            P.stock(w2, [1 if g == w else 0 for g in range(4)])
                        if variant.endswith('limit-1'):
                            f['episode_step'] = np.float64(max_steps - 1 - frame)
                        elif variant.endswith('limit'):
                            f['episode_step'] = np.float64(max_steps - frame)
                        if variant == 'first_delivery':
                            f['num_delivered_cargoes'] = np.float64(0)
                            f['delayed_episode_reward'] = np.float64(0)
                            f['episode_reward'] = np.float64(-17.0)
                        probes.append((t, w, variant, frame, 'deliver', weight))

            P.finish()
            if draws is None and P.Nc:
                P.aim(probes[0][1] if want_tracked and probes else None, {p[1] for p in probes})
            for t, w, rung, frame, expect, detail in probes:
                landing = P.landings[t][0]
                plan.append(Probe(e, kind, t, w, rung, frame, exact_side(*landing), expect, detail, P.tracked(landing), (float(landing[0]), float(landing[1]))))
            for k in PLANTED_KEYS:
                out[k][e] = P.f[k]
            actions[e], goal_u[e] = P.actions, P.goal_u
        scenes.append(Scene(out, actions, goal_u, plan))
    return scenes


def probes_at(plan, env):
    return [p for p in plan if p.env == env]


def describe(probes):
    return ['%s target %d warehouse %d %s frame %d (%s, %s)' % (p.kind, p.target, p.warehouse, p.rung, p.frame, 'inside' if p.side < 0 else 'outside', p.expect)
            for p in probes]


def entries(p):
    """The catalogue entries a probe stands for (what the census of tests/test_logistics_scenes_cpu.py counts)."""
    if p.kind == 'delivery':
        weight, bounty = p.rung.split(' bounty ')
        return [(p.kind, weight), (p.kind, 'bounty ' + bounty)]
    return [(p.kind, p.detail if p.kind == 'shared' else p.rung)]


def catalogue(Nt):
    """Every entry a shape with Nt targets must hold."""
    out = [('rim', r) for r in RIM_RUNGS] + [('carry', '%s %s' % (c, s)) for c in CARRIES for s in ('stocked', 'empty')]
    out += [('delivery', 'weight 1'), ('delivery', 'weight 2')] + [('delivery', 'bounty ' + b) for b in BOUNTIES]
    out += [('shared', v) for v in SHARED if Nt >= 3 or v != 'three_for_two'] + [('pick', name) for name, _, _, _ in PICKS] + [('end', v) for v in END]
    return out


# ------------------------------------------------------------------ the oracle's side of a scene
COMPARED_EXACT = LOGISTICS_KEYS            # integers and integer-valued sums: exact on both sides


def oracle_step(side, tgt_act=None, goal_u=None, cam_act=None, draws=False, live=None):
    """One step of every environment still `live` ([n] bool; default: all) on f64 joint actions (default: zero), the goal tape
    `goal_u` [n, Nt] (None: the environment's own Philox stream) and no see-through draws (`draws`: those of the stream)."""
    zeros = None if draws else np.zeros((max(side.Nc, 1), side.Nt))
    for e, env in enumerate(side.envs):
        if live is not None and not live[e]:
            continue
        env.step(np.zeros((side.Nc, 2)) if cam_act is None else cam_act[e], np.zeros((side.Nt, 2)) if tgt_act is None else tgt_act[e],
                 zeros, None if goal_u is None else goal_u[e])


SCALARS = ('reward_cam', 'reward_tgt', 'done', 'coverage_rate', 'real_coverage_rate', 'mean_transport_rate', 'num_delivered_cargoes', 'normalized_reward_tgt')


def oracle_scalars(side):
    """[n, 8]: the scalar row of the engine (engine.py: SCALAR_NAMES) as the oracle has it."""
    return np.stack([side.batch.gather(k) for k in SCALARS], axis=1)
