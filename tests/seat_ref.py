"""NumPy restatement of the reference's GreedyCameraAgent / GreedyTargetAgent teams of ONE environment (mate/agents/greedy.py) with an optional absent
seat per team -- the slot a learner plays under SingleCamera / SingleTarget (mate/wrappers/single_team.py:310-470) -- in the order of mate.group_step:
observe -> send -> receive -> act, f64.  It takes the tapes oracle.GreedyPolicies.act takes; with no seat it is that restatement again
(tests/test_seat_host.py holds the two together, closed loop).

Around an absent camera seat z: every teammate still sends its one 'state' message to z and draws that pair's delay (the send loop skips only the sender's
own index); z never answers, so it never becomes a neighbour and no later message to it has content.  z sends nothing, draws nothing, keeps no memory.
An absent target seat broadcasts nothing and holds no warehouse set; the teammates' broadcasts reach every slot.  The seat's action rows read NaN."""
import numpy as np

MEMORY_PERIOD = 25            # greedy.py:21
NOISE_SCALE = 0.5             # greedy.py:236
WAREHOUSES = np.array([[925.0, 925.0], [-925.0, 925.0], [-925.0, -925.0], [925.0, -925.0]])      # constants.py:70-72
STATE_BIT = 1 << 31


def normalize_angle(a):
    return (a + 180.0) % 360.0 - 180.0


def sin_deg(x):
    return np.sin(np.deg2rad(x))


def view_of_oracle(env):
    """What the agents of an oracle environment may know, as act() takes it."""
    Nc, Nt = env.Nc, env.Nt
    g = env.get
    return dict(episode=int(g('episode')), m_ct=g('camera_target_view_mask').reshape(Nc, Nt) != 0 if Nc else np.zeros((0, Nt), dtype=bool),
                tgt_xy=np.stack([g('tgt_x'), g('tgt_y')], axis=1), cam_xy=np.stack([g('cam_x'), g('cam_y')], axis=1) if Nc else np.zeros((0, 2)),
                cam_phi=g('cam_phi'), cam_theta=g('cam_theta'), cam_sight=g('cam_sight'), cam_rmax=g('cam_max_sight_range'),
                cam_rot=g('cam_rotation_step'), cam_zoom=g('cam_zooming_step'), tgt_step=g('tgt_step_size'),
                goals=g('tgt_goals').astype(np.int64), empty_bits=g('tgt_empty_bits').reshape(Nt, 4) != 0)


class SeatAgents:
    """Both teams' Greedy agents of one environment.  `integers()`: the agents' integer memory, for comparisons."""

    def __init__(self, Nc, Nt):
        self.Nc, self.Nt = Nc, Nt
        self.episode = -1
        self.mem = np.zeros((Nc, Nt, 2))
        self.t2f = np.zeros((Nc, Nt), dtype=np.int64)
        self.prev_action = np.zeros((Nc, 2))
        self.delay = np.zeros((Nc, Nc), dtype=np.int64)          # [sender][recipient]
        self.neighbor = np.zeros((Nc, Nc), dtype=np.int64)       # [camera][teammate]
        self.has_state = np.zeros(Nc, dtype=np.int64)
        self.tgt_prev = np.zeros((Nt, 2))
        self.tgt_noise = np.zeros((Nt, 2))
        self.tgt_goal = np.zeros(Nt, dtype=np.int64)
        self.tgt_nonempty = np.zeros(Nt, dtype=np.int64)
        self.tgt_need = np.zeros(Nt, dtype=np.int64)

    def reset_memory(self, team):
        """The team's agents run agent.reset at their next call whatever the episode (the engine's mark: enabling, changing or disabling a seat)."""
        self.episode_mark = getattr(self, 'episode_mark', set()) | {team}

    def integers(self):
        return dict(t2f=self.t2f.copy(), delay=self.delay.copy(), neighbor=self.neighbor.copy(), has_state=self.has_state.copy(),
                    tgt_goal=self.tgt_goal.copy(), tgt_nonempty=self.tgt_nonempty.copy(), tgt_need=self.tgt_need.copy())

    def act(self, v, cam_binom_u, cam_sample_u, cam_delay, tgt_choice_u, tgt_binom_u, tgt_sample_u, tgt_reset_sample_u, seat_c=None, seat_t=None,
            cameras=True, targets=True):
        """One acting call on the view `v` (view_of_oracle).  seat_c / seat_t: the absent camera / target slot (None: nobody).  cameras / targets: whether
        the team acts at all.  Returns (cam_act [Nc, 2], tgt_act [Nt, 2], info): NaN rows for a seat and for a team that does not act; info counts
        `state_to_seat` ('state' messages sent to the camera seat), `told` (tracking decisions on a target known only from a message), `broadcasts`
        (target broadcasts) and `sent` [Nc, Nc] / `delay_drawn` [Nc, Nc]."""
        Nc, Nt = self.Nc, self.Nt
        marks = getattr(self, 'episode_mark', set())
        fresh = self.episode != v['episode']
        fresh_c, fresh_t = fresh or 0 in marks, fresh or 1 in marks
        self.episode_mark = set()
        m_ct, txy, cxy = v['m_ct'], v['tgt_xy'], v['cam_xy']
        info = dict(state_to_seat=0, told=0, broadcasts=0, sent=np.zeros((Nc, Nc), dtype=bool), delay_drawn=np.zeros((Nc, Nc), dtype=bool))
        cam_act, tgt_act = np.full((Nc, 2), np.nan), np.full((Nt, 2), np.nan)
        # ---- reset (greedy.py:43-61, 262-283) and observe / process_messages (:100-113, :326-332)
        if cameras:
            for c in range(Nc):
                if c == seat_c:
                    if fresh_c:
                        self.has_state[c] = 0
                        self.delay[c, :] = 0
                        self.neighbor[c, :] = 0
                    continue
                if fresh_c:
                    self.mem[c] = np.where(m_ct[c][:, None], txy, 0.0)
                    self.t2f[c] = np.where(m_ct[c], MEMORY_PERIOD, 0)
                    self.prev_action[c] = 0.0
                    self.delay[c, :] = 0
                    self.neighbor[c, :] = 0
                    self.has_state[c] = 1
                left = np.maximum(self.t2f[c] - 1, 0)
                self.t2f[c] = np.where(m_ct[c], MEMORY_PERIOD, left)
                self.mem[c] = np.where(m_ct[c][:, None], txy, self.mem[c])
        if targets:
            for t in range(Nt):
                if t == seat_t:
                    continue
                step = v['tgt_step'][t]
                if fresh_t:
                    self.tgt_prev[t] = txy[t]
                    self.tgt_noise[t] = 0.5 * (-step + (2.0 * step) * np.asarray(tgt_reset_sample_u[t], dtype=np.float64))
                    self.tgt_goal[t] = v['goals'][t]
                    self.tgt_nonempty[t] = 0xf
                    self.tgt_need[t] = 0
                seen_empty = sum(int(v['empty_bits'][t][w]) << w for w in range(4))
                if seen_empty & self.tgt_nonempty[t]:
                    self.tgt_nonempty[t] &= ~seen_empty
                    self.tgt_need[t] = 1
        if cameras or targets:
            self.episode = v['episode']
        # ---- cameras: send_responses (:158-190)
        if cameras:
            send = np.zeros((Nc, Nc), dtype=np.int64)
            known_before = self.t2f > 0
            for s in range(Nc):
                if s == seat_c:
                    continue                                    # the learner's own messages are not provided
                seen_now = m_ct[s]
                has_content = bool(self.has_state[s]) or seen_now.any()
                for c in range(Nc):
                    d = max(self.delay[s, c] - 1, 0)
                    bits = 0
                    if has_content and s != c and d == 0:
                        if seen_now.any() and self.neighbor[s, c]:      # filterout_beyond_range
                            threshold = 1.1 * v['cam_rmax'][c]
                            for t in range(Nt):
                                if seen_now[t] and np.hypot(txy[t, 0] - cxy[c, 0], txy[t, 1] - cxy[c, 1]) < threshold:
                                    bits |= 1 << t
                        if self.has_state[s]:
                            bits |= STATE_BIT
                        if bits:
                            d = int(cam_delay[s][c])
                            info['sent'][s, c] = info['delay_drawn'][s, c] = True
                            if c == seat_c:
                                assert bits == STATE_BIT      # the seat is nobody's neighbour: 'state' and nothing else, once
                                info['state_to_seat'] += 1
                    self.delay[s, c] = d
                    send[s, c] = bits
            # ---- cameras: receive_responses (:192-226), then message2send.clear()
            told_now = np.zeros((Nc, Nt), dtype=bool)
            for c in range(Nc):
                if c == seat_c:
                    continue
                for s in range(Nc):
                    bits = int(send[s, c])
                    if bits & STATE_BIT:
                        self.neighbor[c, s] = 1
                    for t in range(Nt):
                        if (bits >> t) & 1:
                            self.mem[c, t] = txy[t]
                            self.t2f[c, t] = MEMORY_PERIOD
                            told_now[c, t] = True
            self._told = np.where(m_ct, False, getattr(self, '_told', np.zeros((Nc, Nt), dtype=bool)) | (told_now & ~known_before))
            self._told &= self.t2f > 0
            for c in range(Nc):
                if c != seat_c and (self.has_state[c] or m_ct[c].any()):
                    self.has_state[c] = 0
        # ---- targets: broadcast the non-empty sets (:334-358)
        if targets:
            senders = [s for s in range(Nt) if s != seat_t and self.tgt_need[s]]
            info['broadcasts'] = len(senders)
            sets = self.tgt_nonempty.copy()
            for t in range(Nt):
                if t == seat_t:
                    continue
                for s in senders:
                    sets[t] &= self.tgt_nonempty[s]
            for t in range(Nt):
                if t != seat_t:
                    self.tgt_nonempty[t] = sets[t]
                    self.tgt_need[t] = 0
        # ---- cameras: act (:69-156)
        if cameras:
            for c in range(Nc):
                if c == seat_c:
                    continue
                phi = np.deg2rad(v['cam_phi'][c])
                ox, oy = v['cam_sight'][c] * np.cos(phi), v['cam_sight'][c] * np.sin(phi)
                sight, orientation = np.hypot(ox, oy), np.rad2deg(np.arctan2(oy, ox))      # what the agent derives from its observation row
                theta, rmax = v['cam_theta'][c], v['cam_rmax'][c]
                q2 = sight / rmax
                min_va = theta * (q2 * q2)
                threshold = 1.1 * rmax
                best, best_d = -1, 0.0
                for t in range(Nt):
                    if self.t2f[c, t] <= 0:
                        continue
                    dnorm = np.hypot(self.mem[c, t, 0] - cxy[c, 0], self.mem[c, t, 1] - cxy[c, 1])
                    if not dnorm < threshold:
                        continue
                    if best < 0 or dnorm < best_d:
                        best, best_d = t, dnorm
                if best >= 0:
                    info['told'] += int(self._told[c, best])
                    rx, ry = self.mem[c, best, 0] - cxy[c, 0], self.mem[c, best, 1] - cxy[c, 1]
                    best_orientation = np.rad2deg(np.arctan2(ry, rx))
                    distance = best_d
                    if distance * (1.0 + sin_deg(min_va / 2.0)) >= rmax:
                        best_va = min_va
                    else:
                        area_product = theta * (sight * sight)
                        if distance <= np.sqrt(area_product / 180.0) / 2.0:
                            best_va = 180.0
                        else:
                            b = 180.0
                            for _ in range(20):
                                sr = distance * (1.0 + sin_deg(min(b / 2.0, 90.0)))
                                b = area_product / (sr * sr)
                            best_va = min(max(b, min_va), 180.0)
                    a0 = min(max(normalize_angle(best_orientation - orientation), -v['cam_rot'][c]), v['cam_rot'][c])
                    a1 = min(max(best_va - theta, -v['cam_zoom'][c]), v['cam_zoom'][c])
                elif cam_binom_u[c] > 1.0 - 0.1:                # np_random.binomial(1, 0.1)
                    a0 = -v['cam_rot'][c] + (2.0 * v['cam_rot'][c]) * cam_sample_u[c][0]
                    a1 = -v['cam_zoom'][c] + (2.0 * v['cam_zoom'][c]) * cam_sample_u[c][1]
                else:
                    a0, a1 = self.prev_action[c]
                self.prev_action[c] = (a0, a1)
                cam_act[c] = (a0, a1)
        # ---- targets: act (:285-324)
        if targets:
            for t in range(Nt):
                if t == seat_t:
                    continue
                state_goal, step_size = int(v['goals'][t]), v['tgt_step'][t]
                goal = int(self.tgt_goal[t])
                if state_goal >= 0:
                    goal = state_goal
                nonempty = int(self.tgt_nonempty[t])
                if goal < 0 or (state_goal < 0 and not (nonempty >> goal) & 1):
                    goal = -1
                    members = [w for w in range(4) if (nonempty >> w) & 1]
                    if members:                                 # np_random.choice(list(non_empty_warehouses))
                        goal = members[min(int(tgt_choice_u[t] * len(members)), len(members) - 1)]
                self.tgt_goal[t] = goal
                x, y = txy[t]
                pax, pay = x - self.tgt_prev[t, 0], y - self.tgt_prev[t, 1]
                ax = ay = 0.0
                if goal >= 0:
                    ax, ay = WAREHOUSES[goal][0] - x, WAREHOUSES[goal][1] - y
                length = np.hypot(ax, ay)
                if length > step_size:
                    k2 = step_size / length
                    ax, ay = ax * k2, ay * k2
                prob = 0.05 if np.hypot(pax, pay) > 0.2 * step_size else 0.75
                u = tgt_binom_u[t]
                nx, ny = self.tgt_noise[t]
                if (u > 1.0 - prob) if prob <= 0.5 else (u <= prob):
                    nx = NOISE_SCALE * (-step_size + (2.0 * step_size) * tgt_sample_u[t][0])
                    ny = NOISE_SCALE * (-step_size + (2.0 * step_size) * tgt_sample_u[t][1])
                tgt_act[t] = (min(max(ax + nx, -step_size), step_size), min(max(ay + ny, -step_size), step_size))
                self.tgt_prev[t] = (x, y)
                self.tgt_noise[t] = (nx, ny)
        return cam_act, tgt_act, info


def view_of_fixture(fx, s):
    """The view of what the agents act on at step s: the state the reset (s = 0) or step s - 1 left."""
    pick = (lambda k: fx['reset/' + k]) if s == 0 else (lambda k: fx['step/' + k][s - 1])
    return dict(episode=1, m_ct=pick('camera_target_view_mask') != 0, tgt_xy=pick('tgt_xy'), cam_xy=fx['static/cam_xy'], cam_phi=pick('cam_phi'),
                cam_theta=pick('cam_theta'), cam_sight=pick('cam_sight'), cam_rmax=fx['static/cam_max_sight_range'], cam_rot=fx['static/cam_rotation_step'],
                cam_zoom=fx['static/cam_zooming_step'], tgt_step=fx['static/tgt_step_size'], goals=pick('tgt_goals').astype(np.int64),
                empty_bits=pick('tgt_empty_bits') != 0)


def replay(fx):
    """The agents over a seat fixture (tests/golden/seat_*.npz), the recorded draws on the tape: (worst |teammate / opponent action - recorded|, summed info)."""
    Nc, Nt = int(fx['num_cameras']), int(fx['num_targets'])
    camera = str(fx['seat/team']) == 'camera'
    z = int(fx['seat/index'])
    agents = SeatAgents(Nc, Nt)
    worst, total = 0.0, dict(state_to_seat=0, told=0, broadcasts=0)
    for s in range(len(fx['step/done'])):
        a = lambda k: fx['step/agent_' + k][s]  # noqa: E731
        cam, tgt, info = agents.act(view_of_fixture(fx, s), a('cam_binom_u'), a('cam_sample_u'), a('cam_delay'), a('tgt_choice_u'), a('tgt_binom_u'), a('tgt_sample_u'),
                                    fx['agent/tgt_reset_sample_u'], seat_c=z if camera else None, seat_t=None if camera else z)
        assert np.array_equal(info['delay_drawn'], a('cam_delay') >= 0), ('the delays drawn', s)
        for got, key in ((cam, 'step/cam_act'), (tgt, 'step/tgt_act')):
            rows = np.isfinite(got[:, 0])
            assert rows.sum() == len(got) - (1 if (key == 'step/cam_act') == camera else 0)
            if rows.any():
                worst = max(worst, float(np.abs(got[rows] - fx[key][s][rows]).max()))
        for k in total:
            total[k] += info[k]
    return worst, total


def seat_draw(seed, env_global, episode, team, n, philox):
    """The DRAW formula of csrc/seat_rows.hpp with `philox` = oracle.philox: stream 27, sub = team, word .x scaled to [0, n)."""
    x = philox(seed & 0xffffffff, seed >> 32, env_global, episode, 27, team)[0]
    return (int(x) * n) >> 32


def tape_seats(n_envs, n):
    """Seats for a batch that cover 0, a middle slot and n - 1."""
    return np.array([(0, n // 2, n - 1)[e % 3] for e in range(n_envs)], dtype=np.int32)


def few_cargoes(remaining, goal_bits, goals):
    """The state injection of the few-cargo fixtures for one environment: only the cargoes in transit are left.  Returns (remaining, awaiting)."""
    awaiting = np.zeros(4)
    for t, g in enumerate(np.asarray(goals).astype(int)):
        if g >= 0:
            awaiting[g] += np.asarray(goal_bits).reshape(len(goals), 4)[t, g]
    return np.zeros_like(np.asarray(remaining, dtype=np.float64)), awaiting


def closed_loop(O, batch, team, seats, steps, seed, step_engine=None, agents=None):
    """SeatAgents + the oracle environments of `batch` (reset, occlusion tables set), closed loop on random tapes with a uniformly random learner in seat
    seats[e] of `team` (0 cameras, 1 targets).  `step_engine(tape, action, tape_ct, goal_u) -> (cam_act [n, Nc, 2], tgt_act [n, Nt, 2])` runs the device beside
    it: its joint actions are compared row by row (the seat's row with the learner's action), and the oracle steps on the REFERENCE's rows.  `agents`: the
    SeatAgents to go on with (default: new ones).  Returns (worst difference, summed info)."""
    n = len(seats)
    envs = [batch.env(e) for e in range(n)]
    Nc, Nt = envs[0].Nc, envs[0].Nt
    agents = agents if agents is not None else [SeatAgents(Nc, Nt) for _ in range(n)]
    rng = np.random.RandomState(seed)
    reset_u = rng.random_sample((n, Nt, 2))
    worst, total = 0.0, dict(state_to_seat=0, told=0, broadcasts=0, sent=0)
    for s in range(steps):
        t = {'camera_resample_u': rng.random_sample((n, max(Nc, 1))), 'camera_sample_u': rng.random_sample((n, max(Nc, 1), 2)),
             'camera_delay': rng.randint(6, 50, size=(n, max(Nc, 1), max(Nc, 1))).astype(np.int32),
             'target_choice_u': rng.random_sample((n, Nt)), 'target_resample_u': rng.random_sample((n, Nt)),
             'target_sample_u': rng.random_sample((n, Nt, 2)), 'target_reset_sample_u': reset_u}
        tape_ct, goal_u = rng.random_sample((n, max(Nc, 1), Nt)), rng.random_sample((n, Nt))
        u = rng.uniform(-1.0, 1.0, size=(n, 2))
        if team == 0:
            action = u * np.stack([[envs[e].get('cam_rotation_step')[seats[e]], envs[e].get('cam_zooming_step')[seats[e]]] for e in range(n)])
        else:
            action = u * np.array([envs[e].get('tgt_step_size')[seats[e]] for e in range(n)])[:, None]
        got = step_engine(t, action, tape_ct, goal_u) if step_engine is not None else None
        for e in range(n):
            z = int(seats[e])
            ca, ta, info = agents[e].act(view_of_oracle(envs[e]), t['camera_resample_u'][e, :Nc], t['camera_sample_u'][e, :Nc], t['camera_delay'][e, :Nc, :Nc],
                                         t['target_choice_u'][e], t['target_resample_u'][e], t['target_sample_u'][e], reset_u[e],
                                         seat_c=z if team == 0 else None, seat_t=z if team == 1 else None)
            (ca if team == 0 else ta)[z] = action[e]
            if got is not None:
                worst = max(worst, float(np.abs(ta - got[1][e]).max()), float(np.abs(ca - got[0][e]).max()) if Nc else 0.0)
            for k in ('state_to_seat', 'told', 'broadcasts'):
                total[k] += info[k]
            total['sent'] += int(info['sent'].sum())
            envs[e].step(ca, ta, tape_ct[e, :Nc] if Nc else None, goal_u[e])
    return worst, total
