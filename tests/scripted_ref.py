"""Batched NumPy restatement of the scripted opponents of csrc/scripted_rows.hpp -- NaiveCameraAgent / NaiveTargetAgent (mate/agents/naive.py),
RandomCameraAgent / RandomTargetAgent (mate/agents/random.py) and the per-episode mixture (mate/agents/mixture.py) -- with the reference's operations
in the reference's order, f64.  Pure functions over arrays with a leading batch axis; ScriptedTeam carries one team's memory through a run.

Every result comes with `margin`, per entry the smallest relative distance of a DISCONTINUOUS branch condition from equality (the arrival rule and the
choice of the noise probability; a uniform compared with a constant is exact on both sides, the cut to step_size and the clip are continuous), and
`exact`, where the expected row involves no arithmetic that may round differently on the device (everything but the Naive targets)."""
import numpy as np

SCRIPTED_AGENTS = ('greedy', 'heuristic', 'naive', 'random', 'external')
GREEDY, HEURISTIC, NAIVE, RANDOM, EXTERNAL = range(5)
WAREHOUSES = np.array([[925.0, 925.0], [-925.0, 925.0], [-925.0, -925.0], [925.0, -925.0]])      # constants.py:70-72
WAREHOUSE_RADIUS = 75.0


def mixture_choice(weights, u):
    """RandomState.choice(p=w / sum w) of mixture.py:108 over the candidates with positive weight: searchsorted(cumsum(p), u, side='right').
    Returns indices into the POSITIVE candidates."""
    w = np.asarray(weights, dtype=np.float64)
    w = w[w > 0.0]
    p = w / w.sum()
    k = np.searchsorted(np.cumsum(p), np.asarray(u, dtype=np.float64), side='right')
    return np.minimum(k, len(p) - 1)


def binomial1(prob, u):
    """The mapping of a uniform to np_random.binomial(1, prob) the engine and the fixtures' recording proxy share (tests/golden/make_golden.py: AgentRNG)."""
    return np.where(prob <= 0.5, u > 1.0 - prob, u <= prob)


def naive_camera(u, rotation_step, zooming_step):
    """naive.py:27: np_random.uniform(0.0, 0.4) * action_space.high."""
    m = 0.0 + 0.4 * np.asarray(u, dtype=np.float64)
    return np.stack([m * rotation_step, m * zooming_step], axis=-1)


def box_sample(u, high):
    """action_space.sample() of the recording stand-in: low + (high - low) u with low = -high; `high` broadcasts against u[..., k]."""
    high = np.asarray(high, dtype=np.float64)
    return -high + (2.0 * high) * np.asarray(u, dtype=np.float64)


def naive_target_reset(xy, step_size, reset):
    """naive.py:56-68 from the recorded draws reset[..., 4] = (u0, u1, goal, inc)."""
    s = np.asarray(step_size, dtype=np.float64)[..., None]
    reset = np.asarray(reset, dtype=np.float64)
    return dict(goal=np.nan_to_num(reset[..., 2]).astype(np.int64), inc=np.nan_to_num(reset[..., 3]).astype(np.int64), prev_location=np.array(xy, dtype=np.float64),
                prev_noise=0.5 * box_sample(reset[..., :2], s))


def naive_target_act(mem, xy, step_size, carries, empty_bits, u):
    """naive.py:70-105 for entries [...]: `mem` as naive_target_reset returns it (updated in a copy), `carries` goal_bits.any(), `empty_bits` the four
    empty flags as an integer, u[..., 3] = (binomial u, sample u0, sample u1).  Returns (action, new memory, info)."""
    xy = np.asarray(xy, dtype=np.float64)
    s = np.asarray(step_size, dtype=np.float64)
    goal, inc = mem['goal'].copy(), mem['inc']
    empty = np.asarray(empty_bits, dtype=np.int64)
    dist = np.linalg.norm(xy - WAREHOUSES[goal], axis=-1)
    rim = 0.9 * WAREHOUSE_RADIUS
    arrived = dist <= rim
    margin = np.abs(dist - rim) / rim
    single = np.asarray(carries, dtype=bool) | (empty == 0xf)
    once = arrived & single
    skip = arrived & ~single
    nxt = (goal + inc) % 4
    skipped = np.zeros(goal.shape, dtype=np.int64)
    walk = nxt.copy()
    for _ in range(3):                                   # until a warehouse not known to be empty (at most three more increments)
        more = skip & (((empty >> walk) & 1) == 1)
        walk = np.where(more, (walk + inc) % 4, walk)
        skipped += more
    goal = np.where(once, nxt, np.where(skip, walk, goal))
    action = WAREHOUSES[goal] - xy
    length = np.linalg.norm(action, axis=-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        action = np.where((length > s)[..., None], action * (s / length)[..., None], action)
    moved = np.linalg.norm(xy - mem['prev_location'], axis=-1)
    edge = 0.2 * s
    prob = np.where(moved > edge, 0.05, 0.75)
    margin = np.minimum(margin, np.abs(moved - edge) / edge)
    resample = binomial1(prob, u[..., 0])
    noise = np.where(resample[..., None], 0.5 * box_sample(u[..., 1:3], s[..., None]), mem['prev_noise'])
    out = np.clip(action + noise, -s[..., None], s[..., None])
    new = dict(goal=goal, inc=inc, prev_location=xy.copy(), prev_noise=noise)
    info = dict(margin=margin, once=once, skip=skip, skipped=skipped, prob=prob, resample=resample)
    return out, new, info


class ScriptedTeam:
    """One team's memory under a mixture, as scripted_opponent_kernel keeps it: per environment the episode tag, the kind held, the Random agents' call counter
    and previous action, and the Naive targets' memory.  `team`: 0 cameras, 1 targets; `high` [N, n, 2] the action box (rotation_step, zooming_step) or
    the targets' step sizes twice."""

    def __init__(self, team, num_envs, agents, frame_skip=20):
        self.team, self.N, self.n, self.frame_skip = team, num_envs, agents, frame_skip
        self.episode = np.full(num_envs, -1, dtype=np.int64)
        self.choice = np.full(num_envs, -1, dtype=np.int64)
        self.counter = np.zeros(num_envs, dtype=np.int64)
        self.prev_action = np.zeros((num_envs, agents, 2))
        self.naive = dict(goal=np.zeros((num_envs, agents), dtype=np.int64), inc=np.ones((num_envs, agents), dtype=np.int64),
                          prev_location=np.zeros((num_envs, agents, 2)), prev_noise=np.zeros((num_envs, agents, 2)))
        self.final = np.zeros((num_envs, agents, 2))

    def step(self, live, episode, choice, rows, high, draws, targets=None):
        """One acting call.  live [N]: the agents' launch did not skip the environment; episode [N]; choice [N]: the kind the record reports (taken at a
        team's first call of an episode, checked to hold otherwise); rows {kind: [N, n, 2]}; draws: the record's arrays of this call -- cameras u [N, Nc, 2];
        targets u [N, Nt, 3] and reset [N, Nt, 4] --; targets: dict(xy, carries, empty_bits).  Returns dict(final, margin, exact, used_u, used_reset, fresh,
        info): used_* are the entries of the record that must be finite (all others NaN)."""
        N, n = self.N, self.n
        live = np.asarray(live, dtype=bool)
        fresh = live & (self.episode != episode)
        held = live & ~fresh
        assert np.array_equal(np.asarray(choice)[held], self.choice[held]), 'the choice holds for the episode'
        self.choice = np.where(fresh, choice, self.choice)
        self.episode = np.where(fresh, episode, self.episode)
        self.counter = np.where(fresh, 0, self.counter)
        kind = self.choice
        sample_now = self.counter % self.frame_skip == 0
        final = self.final.copy()
        margin = np.full((N, n), np.inf)
        exact = np.ones((N, n), dtype=bool)
        u = draws['u']
        used_u = np.zeros(u.shape, dtype=bool)
        used_reset = np.zeros((N, n, 4), dtype=bool)
        info = None
        for k in (GREEDY, HEURISTIC, EXTERNAL):
            sel = live & (kind == k)
            if sel.any():
                final[sel] = rows[k][sel]
        rnd = live & (kind == RANDOM)
        first = 0 if self.team == 0 else 1
        draw = rnd & sample_now
        if draw.any():
            sampled = box_sample(u[..., first:first + 2], high)
            self.prev_action[draw] = sampled[draw]
            used_u[draw, :, first:first + 2] = True
        final[rnd] = self.prev_action[rnd]
        nav = live & (kind == NAIVE)
        if nav.any() and self.team == 0:
            final[nav] = naive_camera(u[..., 0], high[..., 0], high[..., 1])[nav]
            used_u[nav, :, 0] = True
        elif nav.any():
            step_size = high[..., 0]
            start = nav & fresh
            if start.any():
                init = naive_target_reset(targets['xy'], step_size, draws['reset'])
                for key in self.naive:
                    self.naive[key][start] = init[key][start]
                used_reset[start] = True
            with np.errstate(invalid='ignore'):
                out, new, info = naive_target_act(self.naive, targets['xy'], step_size, targets['carries'], targets['empty_bits'], np.nan_to_num(u, nan=0.0))
            for key in self.naive:
                self.naive[key][nav] = new[key][nav]
            final[nav] = out[nav]
            margin[nav] = info['margin'][nav]
            exact[nav] = False
            used_u[nav, :, 0] = True
            used_u[..., 1:3] |= (nav[:, None] & info['resample'])[..., None]
            info = {key: value & nav[:, None] if value.dtype == bool else value for key, value in info.items()}
        self.counter = np.where(live, self.counter + 1, self.counter)
        self.final = final
        return dict(final=final, margin=margin, exact=exact, used_u=used_u, used_reset=used_reset, fresh=fresh, info=info)


def fixture_draws(fx):
    """The recorded draws of a naive_* / random_* fixture in the shapes of the engine's tape, with a leading [T] axis: camera_u [T, Nc, 2], target_u
    [T, Nt, 3], and target_reset [Nt, 4] (NaN for the Random pair, which draws nothing at its reset)."""
    naive = str(fx['policy']) == 'naive'
    T, Nc, Nt = len(fx['step/done']), int(fx['num_cameras']), int(fx['num_targets'])
    if naive:
        camera_u = np.stack([fx['step/agent_cam_uniform_u'], np.full((T, Nc), np.nan)], axis=-1)
        reset = np.concatenate([fx['agent/tgt_reset_sample_u'], fx['agent/tgt_reset_choice'].astype(np.float64)], axis=-1)
    else:
        camera_u = np.asarray(fx['step/agent_cam_sample_u'], dtype=np.float64).reshape(T, Nc, 2)
        reset = np.full((Nt, 4), np.nan)
    target_u = np.concatenate([fx['step/agent_tgt_binom_u'][..., None], fx['step/agent_tgt_sample_u']], axis=-1)
    return dict(camera_u=camera_u, target_u=target_u, target_reset=reset)


def replay_fixture(fx, frame_skip=20, teams=(0, 1)):
    """The restatement over every step of a naive_* / random_* fixture (one environment, both teams the recorded pair): the state the agents of step s
    act on is what the step before, or the reset, left.  Returns the expected actions, the worst difference from the recorded ones, the smallest branch
    margin and the census of the Naive targets' branches.  `teams`: which teams the recorded pair played (an episode of mixture_4v8-9: the targets only)."""
    kind = NAIVE if str(fx['policy']) == 'naive' else RANDOM
    T, Nc, Nt = len(fx['step/done']), int(fx['num_cameras']), int(fx['num_targets'])
    draws = fixture_draws(fx)

    def before(key, s):
        return np.asarray(fx['reset/' + key] if s == 0 else fx['step/' + key][s - 1])
    step_size = np.asarray(fx['static/tgt_step_size'], dtype=np.float64)[None]
    which, teams = teams, [ScriptedTeam(0, 1, Nc, frame_skip), ScriptedTeam(1, 1, Nt, frame_skip)]
    cam_high = np.stack([fx['static/cam_rotation_step'], fx['static/cam_zooming_step']], axis=-1)[None] if Nc else np.zeros((1, 0, 2))
    tgt_high = np.stack([step_size, step_size], axis=-1)
    cam, tgt = np.zeros((T, Nc, 2)), np.zeros((T, Nt, 2))
    census = dict(once=0, skip=0, far=0, p05=0, p75=0)
    margin = np.inf
    live, episode, choice = np.array([True]), np.array([1]), np.array([kind])
    for s in range(T):
        if Nc and 0 in which:
            out = teams[0].step(live, episode, choice, {}, cam_high, dict(u=draws['camera_u'][s][None]))
            cam[s] = out['final'][0]
            assert np.array_equal(np.isfinite(draws['camera_u'][s][None]), out['used_u']), s
        empty = (before('tgt_empty_bits', s) != 0).astype(np.int64) @ np.array([1, 2, 4, 8])
        targets = dict(xy=before('tgt_xy', s)[None], carries=(before('tgt_goal_bits', s) != 0).any(-1)[None], empty_bits=empty[None])
        out = teams[1].step(live, episode, choice, {}, tgt_high, dict(u=draws['target_u'][s][None], reset=draws['target_reset'][None]), targets)
        tgt[s] = out['final'][0]
        assert np.array_equal(np.isfinite(draws['target_u'][s][None]), out['used_u']), s
        margin = min(margin, float(out['margin'].min()))
        if out['info'] is not None:
            info = out['info']
            census['once'] += int(info['once'].sum()); census['skip'] += int(info['skip'].sum()); census['far'] += int((info['skip'] & (info['skipped'] >= 2)).sum())
            census['p05'] += int((info['prob'] == 0.05).sum()); census['p75'] += int((info['prob'] == 0.75).sum())
    worst = max(float(np.abs(cam - fx['step/cam_act']).max()) if Nc and 0 in which else 0.0, float(np.abs(tgt - fx['step/tgt_act']).max()))
    return dict(cam=cam, tgt=tgt, worst=worst, margin=margin, **census)


def mixture_episodes(fx):
    """The episodes of mixture_4v8-9.npz as fixtures of their own (the keys under ep<k>/), in order."""
    out = []
    for k in range(int(fx['episodes'])):
        prefix = f'ep{k}/'
        out.append({key[len(prefix):]: fx[key] for key in fx.keys() if key.startswith(prefix)})
    return out
