"""The occlusion lookup's crowded-cell tiers: synthetic tables and probes shared by tests/test_lookup_tiers_cpu.py (the oracle
alone: is the plan real?) and tests/test_gpu_lookup_tiers.py (every kernel form against the oracle).  Pure NumPy.

Camera.perceive ends in `norm <= sight_range_at(angle) * (1 + 1e-6)` (entities.py:491-511).  sector_resolve (engine_kernels.hpp)
answers it by one of five paths, chosen by the number of knots of the bearing's half-degree cell -- `count`: the knots from the last
one at or below the cell's start through the first one at or above the next cell's start -- and by Ctx::pivots:

    tier   count        pivots true                      pivots false
    T0     <= 5         segment record                   segment record
    T1     6 .. 17      pivot                            quarter
    T2     18 .. 37     pivot                            one narrowing level, quarter
    T3     38 .. 65     one narrowing level, quarter     same
    T4     66 .. 257    two levels                       same
    T5     258 .. 1025  three levels                     same
    T6     >= 1026      lut_lookup                       same
    G      a cell mate_engine_lut_write marks "general" (a repeated angle, a degree whose integer knot is missing): lut_lookup

A table here has the real shape -- a knot on every integer degree from -180, a closing knot at phis[0] + 360 -- with interior knots
inserted into chosen cells so that the cell's count is exactly a chosen value: every count on either side of a threshold, in a cell
that starts on an integer knot ('first'), one that starts at x.5 ('second') and the two seam cells 0 and 719.  Engine.lut_write
installs such a table per (environment, camera) whatever the obstacles are, so a probe stands on a lookup boundary without touching
a circle.  Ranges zigzag between neighbouring knots (a bracket off by one knot moves the limit by more than 1e-3 relative) with an
amplitude that shrinks with the knot spacing, so that offsets of 1e-9 survive the f64 evaluation of the bearing."""
import collections

import numpy as np

import rim_scenes as RS

# engine_kernels.hpp, restated
K_DEG_SLOTS = 5
K_PIVOT_KNOTS = 9 * (K_DEG_SLOTS - 1) + 1          # 37
K_QUARTER_KNOTS = 4 * (K_DEG_SLOTS - 1) + 1        # 17
CELLS = 720
THRESHOLD_COUNTS = (5, 6, 17, 18, 37, 38, 65, 66, 257, 258, 1025, 1026)
TIERS = ('T0', 'T1', 'T2', 'T3', 'T4', 'T5', 'T6', 'G')
CELL_KINDS = ('first', 'second', 'seam0', 'seam719')
EPS_DEG = 1e-9                                      # probes beside a knot or a cell boundary
MAGNITUDES = sorted({abs(d) for d in RS.LOOKUP_DELTAS})
SECTOR_MARGIN, SIGHT_MARGIN = 0.3, 0.01            # a kept probe is decided by the lookup: this far inside the sector (degrees) and the sight range
WALK = 23.0                                         # clearance around a planted arc: a whole step of the random policy and a little


def pivot_stride(count):
    return (count - 1 + 8) // 9


def tier_of(count):
    for tier, top in zip(TIERS, (K_DEG_SLOTS, K_QUARTER_KNOTS, K_PIVOT_KNOTS, 4 * 16 + 1, 4 * 64 + 1, 4 * 256 + 1)):
        if count <= top:
            return tier
    return 'T6'


def cell_start(cell):
    return cell * 0.5 - 180.0


def cell_of(angle):
    return int(min(max(np.floor((angle + 180.0) * 2.0), 0), CELLS - 1))


def cell_counts(phis):
    """(index of the first knot, count) of every half-degree cell: the builders' rule (reset_kernels.hpp, mate_engine_lut_write)."""
    phis = np.asarray(phis, dtype=np.float64)
    starts = np.arange(CELLS) * 0.5 - 180.0
    first = np.searchsorted(phis, starts, side='right') - 1
    end = np.searchsorted(phis, starts + 0.5, side='left')
    return first, end - first + 1


# cell: the planted cell; count: its planned count; kind: CELL_KINDS or a variant ('halfstart', 'repeat', 'missing'); tier: the tier the
# census books it under; first: index of the cell's first knot in the table
Plant = collections.namedtuple('Plant', 'env cam cell count kind tier first')
# bearing: planned, degrees; delta: planned relative offset of the distance from limit * (1 + 1e-6); what: which boundary it stands beside
Probe = collections.namedtuple('Probe', 'env cam tgt bearing delta what plant')
Plan = collections.namedtuple('Plan', 'tables poses plants rounds dropped planned cell_tier')


class _Table:
    """One camera's table while it is built: integer-degree knots at `base`, then inserted cells."""

    def __init__(self, base):
        self.knots = {float(d): base * (1.0 + 0.12 * (-1) ** d) for d in range(-180, 180)}
        self.extra = []                             # a repeated angle cannot live in the dict
        self.general = set()                        # cells the host builder marks "general"

    def fill(self, cell, inserted, mid, amp, lo=0.0, hi=1.0):
        """`inserted` interior knots evenly inside the fraction (lo, hi) of the cell, zigzagging about `mid`; the integer knots around
        the degree take `mid`."""
        a = cell_start(cell)
        deg = np.floor(a)
        self.knots[float(deg)] = mid
        if deg + 1.0 < 180.0:
            self.knots[float(deg + 1.0)] = mid
        elif deg + 1.0 == 180.0:
            self.knots[-180.0] = mid               # the closing knot repeats the first one's range
        for i in range(inserted):
            x = a + 0.5 * (lo + (hi - lo) * (i + 1) / (inserted + 1))
            self.knots[float(x)] = mid + amp * (-1) ** i

    def arrays(self):
        items = sorted(list(self.knots.items()) + self.extra, key=lambda kv: kv[0])
        phis = np.array([k for k, _ in items] + [items[0][0] + 360.0])
        rhos = np.array([v for _, v in items] + [items[0][1]])
        return phis, rhos


def amplitude(sight, inserted):
    """Zigzag amplitude of a cell with `inserted` interior knots: at most 0.03 of the sight range, and a slope of at most 8 sight ranges
    per degree, so that the 1e-14 degrees between two evaluations of a bearing move the limit by 1e-13 relative at most."""
    spacing = 0.5 / (inserted + 1)
    return sight * min(0.03, 8.0 * spacing)


def boundary_knots(count, rng):
    """{local knot index: name} of a cell with `count` knots: the first and the last interior knot and every selection boundary of the
    cell's paths -- the pivot record's q .. 8q, and q, 2q, 3q of each narrowing level and of the final quarter (two of the four
    sub-ranges are followed at every level: an outer and an inner one)."""
    last = count - 1
    out = {}
    if last >= 2:
        out[1], out[last - 1] = 'first interior', 'last interior'
    if count <= K_DEG_SLOTS:
        out.update({i: 'segment' for i in range(1, last)})
        return out
    if count <= K_PIVOT_KNOTS:
        q = pivot_stride(count)
        out.update({i * q: 'pivot %d' % i for i in range(1, 9) if i * q <= last})
    if count > 4 * 256 + 1:
        out.update({int(i): 'search' for i in np.linspace(2, last - 2, 12)})
        return out

    def walk(start, cnt, level):
        q, lst = (cnt + 2) // 4, cnt - 1
        name = 'quarter' if cnt <= K_QUARTER_KNOTS else 'level %d' % level
        for i in (1, 2, 3):
            out.setdefault(start + min(i * q, lst), '%s %dq' % (name, i))
        if cnt <= K_QUARTER_KNOTS:
            return
        subs = [(b, min(q + 1, cnt - b)) for b in (0, q, 2 * q, 3 * q) if cnt - b >= 2]
        picks = {0 if rng.randint(2) else len(subs) - 1, 1 + rng.randint(2) if len(subs) == 4 else 0}
        for k in picks:
            walk(start + subs[k][0], subs[k][1], level + 1)

    walk(0, count, 1)
    return {k: v for k, v in out.items() if 0 < k <= last}


def planned_bearings(phis, plant, rng):
    """[(bearing, what)] of a plant: each boundary knot at -/+ 1e-9 degrees and at the midpoint to the next knot, and the cell's start and
    end at -/+ 1e-9."""
    out = []
    if plant.kind in ('repeat', 'missing'):
        _, counts = cell_counts(phis)
        local = {i: 'interior' for i in range(1, int(counts[plant.cell]))}
    else:
        local = boundary_knots(plant.count, rng)
    a = cell_start(plant.cell)
    for k, what in sorted(local.items()):
        j = plant.first + k
        if j + 1 >= len(phis) or not a <= phis[j] <= a + 0.5:
            continue
        out += [(phis[j] - EPS_DEG, what + ' -'), (phis[j] + EPS_DEG, what + ' +')]
        if phis[j + 1] > phis[j]:                   # (between the two knots of a repeated angle there is no bearing)
            out.append((0.5 * (phis[j] + phis[j + 1]), what + ' mid'))
    out += [(a - EPS_DEG, 'cell start -'), (a + EPS_DEG, 'cell start +'), (a + 0.5 - EPS_DEG, 'cell end -'), (a + 0.5 + EPS_DEG, 'cell end +')]
    return [(float(RS._norm_angle(b)), what) for b, what in out]


def _recipes():
    """The tables of a batch: [(aim, [(cell offset from the aimed cell, count or variant)])].  aim 'in': the camera looks towards the
    middle of the terrain, and the cell offsets are from the first cell of that degree; aim 'west': it looks at the seam, and the cells
    are absolute.  One large tier per table."""
    big = [c for c in THRESHOLD_COUNTS if c > 66]
    small = [c for c in THRESHOLD_COUNTS if c <= 66]
    out = []
    for i, c in enumerate(big):                     # first-half and second-half cells: one large and two small counts per table
        for half in (0, 1):
            s0, s1 = small[(2 * i + half) % len(small)], small[(2 * i + half + 4) % len(small)]
            out.append(('in', [(half, c), (8 + (1 - half), s0), (-8 + half, s1)]))
    for i, c in enumerate(small):                   # ... so that every small count has both kinds as well
        out.append(('in', [(0, c), (9, small[(i + 3) % len(small)]), (-7, small[(i + 5) % len(small)])]))
    out += [('in', [(0, 'halfstart'), (8, 'repeat')]), ('in', [(0, 'missing'), (9, 'repeat')])]
    counts = list(THRESHOLD_COUNTS)
    for c0, c719 in zip(counts, reversed(counts)):  # the seam cells: (5, 1026), (6, 1025), ... (1026, 5)
        out.append(('west', [(0, c0), (CELLS - 1, c719)]))
    return out


def _aim(env, c, aim, rmax, theta_min, zoom):
    """(first cell of the aimed degree, theta, sight range) of camera c looking along `aim`, or None where the terrain is too short."""
    cx, cy = env.cam[c]
    deg = -180 if aim == 'west' else int(np.floor(np.rad2deg(np.arctan2(-cy, -cx))))
    deg = min(max(deg, -170), 169) if aim == 'in' else deg
    u = RS._unit(deg + 0.25)
    reach = min(((np.sign(u[k]) * (RS.TERRAIN - 1.0) - (cx, cy)[k]) / u[k]) for k in (0, 1) if abs(u[k]) > 1e-9)
    sight = min((reach - WALK - 10.0) / 0.9, rmax * np.sqrt(theta_min / (theta_min + 2.0 * zoom + 1.0)))
    theta = theta_min * rmax * rmax / (sight * sight)
    if theta > 180.0 - 2.0 * zoom - 1.0:
        return None
    return 2 * (deg + 180) % CELLS, float(theta), float(np.sqrt(theta_min * rmax * rmax / theta))


def _clear_mid(env, c, cells, sight, amp, rng):
    """A mid range for the planted cells: the arc of each, `amp` either side of it, is WALK clear of every circle."""
    cam = env.cam[c]
    for frac in rng.permutation(np.linspace(0.3, 0.75, 46)):
        mid = frac * sight
        ok = True
        for b in [cell_start(cell) + x for cell in cells for x in (-0.05, 0.25, 0.55)]:
            u = RS._unit(b)
            ok = ok and env.clear_walk(cam + (mid - amp - 2.0) * u, cam + (mid + amp + 2.0) * u, WALK)
        if ok:
            return float(mid)
    return None


def build_tables(state, cfg, kmax, seed):
    """Synthetic tables for a natively reset `state` ([n, ...] fields): {(env, camera): (phis, rhos)} for the cameras that carry a
    recipe, their poses {(env, camera): (phi, theta)}, the plants and the cells marked general {(env, camera): set}."""
    rng = np.random.RandomState(seed)
    n, Nc = np.shape(state['cam_x'])
    cam_cfg = cfg['camera']
    rmax, theta_min, zoom = float(cam_cfg['max_sight_range']), float(cam_cfg['min_viewing_angle']), float(cam_cfg['zooming_step'])
    todo = _recipes()
    tables, poses, plants, general = {}, {}, [], {}
    slots = [(e, c) for c in range(Nc) for e in range(n)]
    for e, c in slots:
        if not todo:
            break
        env = RS._Env(state, e, cfg, None)
        for r, (aim, cells) in enumerate(todo):
            got = _aim(env, c, aim, rmax, theta_min, zoom)
            if got is None:
                continue
            cell0, theta, sight = got
            table = _Table(0.5 * sight)
            mine, ok, west_mid = [], True, None
            for off, what in cells:
                cell = off if aim == 'west' else (cell0 + off) % CELLS
                if aim == 'in' and not 2 <= cell <= CELLS - 3:
                    ok = False
                    break
                count = what if isinstance(what, int) else {'halfstart': 10, 'repeat': 11, 'missing': 8}[what]
                amp = amplitude(sight, count - 2)
                if aim == 'west':                   # the two seam cells share the knot at -180: one mid range for both
                    west_mid = west_mid or _clear_mid(env, c, [0, CELLS - 1], sight, 0.03 * sight, rng)
                    mid = west_mid
                else:
                    mid = _clear_mid(env, c, [cell - 1, cell, cell + 1] if what == 'missing' else [cell], sight, amp, rng)
                if mid is None:
                    ok = False
                    break
                if what == 'halfstart':             # a knot exactly on x.5: it ends the first-half cell and starts the second-half one
                    cell -= cell % 2
                    table.fill(cell, 8, mid, amp)
                    table.fill(cell + 1, 20, mid, amplitude(sight, 20))
                    table.knots[cell_start(cell + 1)] = mid
                    mine += [(cell, 10, 'halfstart', None), (cell + 1, 22, 'halfstart', None)]
                elif what == 'repeat':              # one angle twice, with a step of the range between the two
                    table.fill(cell, 8, mid, amp)
                    x = sorted(k for k in table.knots if cell_start(cell) < k < cell_start(cell) + 0.5)[3]
                    table.extra.append((x, table.knots[x] + 2.0 * amp))
                    table.general.add(cell)
                    mine.append((cell, 11, 'repeat', 'G'))
                elif what == 'missing':             # a degree without its integer knot: its two cells and the one before it
                    cell -= cell % 2
                    for k in (cell - 1, cell, cell + 1):
                        table.fill(k, 6, mid, amp, 0.1, 0.9)
                    del table.knots[cell_start(cell)]
                    table.general |= {cell - 1, cell, cell + 1}
                    mine += [(k, 8, 'missing', 'G') for k in (cell - 1, cell, cell + 1)]
                else:
                    table.fill(cell, count - 2, mid, amp)
                    kind = 'seam0' if cell == 0 else 'seam719' if cell == CELLS - 1 else ('first', 'second')[cell % 2]
                    mine.append((cell, count, kind, tier_of(count)))
            phis, rhos = table.arrays()
            if not ok or len(phis) > kmax:
                continue
            first, counts = cell_counts(phis)
            for cell, count, kind, tier in mine:
                tier = tier or tier_of(int(counts[cell]))
                plants.append(Plant(e, c, cell, count, kind, tier, int(first[cell])))
            phi = RS._norm_angle(cell_start(cell0) + 0.25 if aim == 'in' else 180.0)
            tables[(e, c)], poses[(e, c)], general[(e, c)] = (phis, rhos), (float(phi), theta), table.general
            del todo[r]
            break
    assert not todo, ('no camera of this batch can carry these tables', todo)
    return tables, poses, plants, general


def full_tables(tables, fallback):
    """[[(phis, rhos)] per camera] per environment: the synthetic table where there is one, `fallback[e][c]` elsewhere."""
    return [[tables.get((e, c), fallback[e][c]) for c in range(len(fallback[e]))] for e in range(len(fallback))]


def realised(cam_xy, point, table):
    """(bearing, relative offset of the distance from the limit * (1 + 1e-6)) at which `point` stands: np.interp on the f64 bearing."""
    rx, ry = point[0] - cam_xy[0], point[1] - cam_xy[1]
    bearing = float(np.rad2deg(np.arctan2(ry, rx)))
    return bearing, float(np.hypot(rx, ry)) / (RS.lut_at(table, bearing) * (1 + 1e-6)) - 1.0


def decided_by_lookup(cam_xy, phi, theta, sight, point):
    """The camera's verdict on `point` is the lookup's: inside the sector by more than 0.3 degrees, inside the sight range by more than 1 %."""
    rx, ry = point[0] - cam_xy[0], point[1] - cam_xy[1]
    ra = abs(phi - float(np.rad2deg(np.arctan2(ry, rx))))
    return min(ra, 360.0 - ra) < 0.5 * theta - SECTOR_MARGIN and float(np.hypot(rx, ry)) < sight * (1.0 - SIGHT_MARGIN)


def kept(probe, planted_delta, fields, cfg, table):
    """The probe still stands on its rim in the state `fields` (f64 [n, ...] arrays): the offset realised there is within a factor 2 of
    the planned one and the verdict is the lookup's."""
    e, c, t = probe.env, probe.cam, probe.tgt
    cam_cfg = cfg['camera']
    cam_xy, point = (fields['cam_x'][e][c], fields['cam_y'][e][c]), (fields['tgt_x'][e][t], fields['tgt_y'][e][t])
    theta = float(fields['cam_theta'][e][c])
    sight = float(np.sqrt(cam_cfg['min_viewing_angle'] * cam_cfg['max_sight_range'] ** 2 / theta))
    _, got = realised(cam_xy, point, table)
    return 0.5 < got / planted_delta < 2.0 and decided_by_lookup(cam_xy, float(fields['cam_phi'][e][c]), theta, sight, point)


def cell_tiers(table, general):
    """The tier of each of the 720 cells of a table; `general`: the cells the host builder marks general."""
    tiers = [tier_of(int(k)) for k in cell_counts(table[0])[1]]
    for cell in general:
        tiers[cell] = 'G'
    return tiers


def probe_tier(probe, fields, plan):
    """The tier of the cell in which the probe's realised bearing lies."""
    e, c, t = probe.env, probe.cam, probe.tgt
    bearing, _ = realised((fields['cam_x'][e][c], fields['cam_y'][e][c]), (fields['tgt_x'][e][t], fields['tgt_y'][e][t]), plan.tables[(e, c)])
    return plan.cell_tier[(e, c)][cell_of(RS._norm_angle(bearing))]


def build_plan(state, cfg, kmax, seed, random_actions=None, max_rounds=None):
    """Tables, camera poses and rounds of probes for a natively reset `state`.  A round is (state fields to plant, [Probe]): every target
    of an environment stands on one probe of one of the environment's tables.  The probes of an environment are dealt round-robin over
    its plants and their boundaries, so that the first few rounds already hold every plant.  `random_actions` = (camera actions
    [n, Nc, 2], target actions [n, Nt, 2]) of the random policy's next step: poses and positions are pre-compensated, so that the probes
    stand on their rims BEHIND that step's kinematics."""
    rng = np.random.RandomState(seed + 1)
    tables, poses, plants, general = build_tables(state, cfg, kmax, seed)
    n, Nt = np.shape(state['tgt_x'])
    cam_cfg = cfg['camera']
    compensated = random_actions is not None
    pending = collections.defaultdict(list)        # env -> [(bearing, delta, what, plant index)], interleaved over the env's plants
    turn = 0
    for e in range(n):
        lists = []
        for i, plant in enumerate(plants):
            if plant.env != e:
                continue
            one = []
            for bearing, what in planned_bearings(tables[(e, plant.cam)][0], plant, rng):
                mag = MAGNITUDES[turn % len(MAGNITUDES)]
                turn += 1
                one += [(bearing, -mag, what, i), (bearing, mag, what, i)]
            order = rng.permutation(len(one) // 2)
            lists.append([one[2 * k + s] for k in order for s in (0, 1)])
        while any(lists):
            for one in lists:
                pending[e] += one[:2]
                del one[:2]
    planned = sum(len(v) for v in pending.values())
    cam_phi, cam_theta = np.array(state['cam_phi'], dtype=np.float64), np.array(state['cam_theta'], dtype=np.float64)
    pose_phi, pose_theta = cam_phi.copy(), cam_theta.copy()
    for (e, c), (phi, theta) in poses.items():
        pose_phi[e, c], pose_theta[e, c] = phi, theta
        act = random_actions[0][e][c].astype(np.float64) if compensated else np.zeros(2)
        cam_phi[e, c], cam_theta[e, c] = RS._norm_angle(phi - act[0]), theta - act[1]
        assert cam_cfg['min_viewing_angle'] < min(theta, cam_theta[e, c]) and max(theta, cam_theta[e, c]) < 180.0
    rounds, dropped = [], 0
    envs = {e: RS._Env(state, e, cfg, None) for e in pending}
    while any(pending.values()) and (max_rounds is None or len(rounds) < max_rounds):
        tx, ty = np.array(state['tgt_x'], dtype=np.float64), np.array(state['tgt_y'], dtype=np.float64)
        probes = []
        for e, queue in pending.items():
            env = envs[e]
            t = 0
            while queue and t < Nt:
                bearing, delta, what, i = queue.pop(0)
                c = plants[i].cam
                table = tables[(e, c)]
                dist = RS.lut_at(table, bearing) * (1 + 1e-6) * (1.0 + delta)
                p = env.cam[c] + dist * RS._unit(bearing)
                walk = RS.clamped(random_actions[1][e][t].astype(np.float64), env.step[t]) if compensated else np.zeros(2)
                start = p - walk
                sight = float(np.sqrt(env.area / pose_theta[e, c]))
                ok = env.free(p) and env.free(start) and env.clear_walk(start, p, 0.05)
                ok = ok and 0.5 < realised(env.cam[c], start + walk, table)[1] / delta < 2.0
                ok = ok and decided_by_lookup(env.cam[c], pose_phi[e, c], pose_theta[e, c], sight, start + walk)
                if not ok:
                    dropped += 1
                    continue
                tx[e, t], ty[e, t] = start
                probes.append(Probe(e, c, t, bearing, delta, what, i))
                t += 1
        rounds.append(({'tgt_x': tx, 'tgt_y': ty, 'cam_phi': cam_phi, 'cam_theta': cam_theta}, probes))
    return Plan(tables, poses, plants, rounds, dropped, planned, {k: cell_tiers(tables[k], general[k]) for k in tables})


# ------------------------------------------------------------------ natural geometry for the device builder (one camera, nine obstacles)
NATURAL_CAMERA = (500.0, 500.0)
NATURAL_RMAX = 2000.0
NATURAL_THETA = 32.0                                # sight range 1936: a shadow's limit is inside it by more than 1 %
NATURAL_N = 192                                     # probes = environments of the one-camera engine


def _row(k, x0, dx, y0, dy, radius):
    i = np.arange(k, dtype=np.float64)
    return np.stack([x0 + dx * i, y0 + dy * i, np.full(k, radius)], axis=1)


# name -> (obstacles [9, 3], the tier of the fullest cell of the camera's table).  Nine obstacles reach 92 knots in a cell at the most
# (ten knots each and the cell's two ends): T5 needs 258, which no geometry of nine obstacles gives.
NATURAL_SCENES = {
    'row_of_nine_r1.5': (_row(9, -300.0, -40.0, -300.0, -40.0, 1.5), 'T4'),
    'fan_of_nine_r4': (_row(9, -600.0, 20.0, -600.0, -15.0, 4.0), 'T2'),
    'rows_of_five_and_four_r1.5': (np.concatenate([_row(5, -300.0, -40.0, -300.0, -40.0, 1.5), _row(4, -300.0, -40.0, 900.0, 10.0, 1.5)]), 'T3'),
    # 32 knots: pivot stride 4, the only stride at which the bracket behind a pivot that sits one knot late falls out of the five fetched
    'row_of_three_and_six_apart_r1.5': (np.concatenate([_row(3, -300.0, -40.0, -300.0, -40.0, 1.5), _row(6, -800.0, 250.0, 900.0, 0.0, 1.5)]), 'T2'),
}


def natural_cell(phis):
    """The fullest cell of a table."""
    return int(np.argmax(cell_counts(phis)[1]))


def natural_phi(phis):
    return float(cell_start(natural_cell(phis)) + 0.25)


def natural_probes(phis, rhos, n=NATURAL_N):
    """n probes [(point, planned delta)] on the fullest cell of a natural table, both sides of the limit: first beside and behind the
    knots boundary_knots names for the cell's count -- the selection boundaries of its lookup path -- then the cell's other knots."""
    table = (np.asarray(phis), np.asarray(rhos))
    cell = natural_cell(phis)
    first, counts = cell_counts(phis)
    first, count = int(first[cell]), int(counts[cell])
    sight = float(np.sqrt(30.0 * NATURAL_RMAX ** 2 / NATURAL_THETA))
    chosen = sorted(k for k in boundary_knots(count, np.random.RandomState(count)) if k < count - 1)
    order = chosen + [k for k in range(1, count - 1) if k not in chosen]
    out, turn = [], 0
    cam = np.array(NATURAL_CAMERA)
    for k in order * len(MAGNITUDES):               # (a short cell comes round again with the next magnitude)
        j = first + k
        for bearing in (phis[j] - EPS_DEG, phis[j] + EPS_DEG, 0.5 * (phis[j] + phis[j + 1])):
            mag = MAGNITUDES[(turn + turn // (3 * len(order))) % len(MAGNITUDES)]
            turn += 1
            pair = []
            for delta in (-mag, mag):
                limit = RS.lut_at(table, bearing)
                p = cam + limit * (1 + 1e-6) * (1.0 + delta) * RS._unit(bearing)
                if limit < 0.98 * sight and np.abs(p).max() < RS.TERRAIN - 1.0 and 0.5 < realised(cam, p, table)[1] / delta < 2.0:
                    pair.append(((float(p[0]), float(p[1])), delta))
            if len(pair) == 2:
                out += pair
    assert len(out) >= n, len(out)
    return out[:n]
