// opponent_host.inc -- the opponents' side of the host, included by mate_engine.hip (which defines fail, HIP_TRY, MATE_TRY, dev_alloc, enter_host and the rest it
// uses).  Host only.  First the launches the two-launch form of step_with_policies puts between the agents' launch and the stepping launch, each reading the call's
// OpponentPlan (engine_host.h); then the setters and accessors of the plain selections, the Heuristic cameras, the mixtures and the channels.

// Between the agents' launch and the stepping launch -- the Heuristic opponents' final joint action from the Greedy one (`freeze_done`: of the agents' launch)
static int launch_drift(mate_engine *e, const OpponentPlan &op, int freeze_done, hipStream_t stream) {
    const DriftArgs a{e->q.tgt_act, e->opponents.d_drift, e->g.own_masks, e->q.noise_scale, e->p.bit_range, freeze_done};
    HIP_TRY(launch_heuristic_drift(op.drift_rows.blocks, op.drift_rows.lds, stream, e->d_params, e->g, a));
    return MATE_OK;
}

// In front of the stepping launch -- the Heuristic camera opponents' joint action, goals and memory (`freeze_done`: of the call).  Identical arguments at
// every call but for the tapes, no allocation, no synchronisation.
static int launch_heuristic_cameras(mate_engine *e, const mate_policy_tape *tape, int freeze_done, hipStream_t stream) {
    CameraOpponent &o = e->camera_opponent;
    const HeuristicCameraArgs a{o.d_mesh, o.d_grid, o.d_scores, e->g.own_masks, o.d_action, o.d_prev, o.d_goals, o.d_index, o.d_episode,
                                tape ? tape->camera_resample_u_dev : nullptr, tape ? tape->camera_sample_u_dev : nullptr, o.permutations, o.record, freeze_done};
    HIP_TRY(launch_heuristic_camera((unsigned)e->N, heuristic_camera_lds_bytes(e->p.Nc), stream, e->d_params, e->g, a));
    o.ran = true;
    return MATE_OK;
}

// Behind the agents' launch and the two Heuristic launches, ahead of the stepping launch -- the Naive and Random agents and the mixtures' choice of the final rows, for the teams the
// engine plays under a mixture (`freeze_done`: of the agents' launch).  Identical arguments at every call but for the team the caller plays, no allocation, no synchronisation.
static ScriptedTeam scripted_team_args(const mate_engine *e, int team, bool plays) {
    const ScriptedMixture &m = e->scripted.team[team];
    ScriptedTeam t{};
    if (!plays) return t;
    t.on = 1; t.count = m.count; t.frame_skip = m.frame_skip; t.n = agents_of(e, team);
    for (int i = 0; i < kScriptedKinds; ++i) { t.kinds[i] = m.kinds[i]; t.cum[i] = m.cum[i]; }
    t.rows[SCRIPTED_GREEDY] = rows_of(e, team, ROWS_GREEDY);
    t.rows[SCRIPTED_HEURISTIC] = rows_of(e, team, ROWS_HEURISTIC);
    t.rows[SCRIPTED_EXTERNAL] = m.d_external;
    t.final_act = m.d_final; t.episode = m.d_episode; t.choice = m.d_choice; t.counter = m.d_counter; t.prev_action = m.d_prev_action;
    t.goal = m.d_goal; t.inc = m.d_inc; t.prev_location = m.d_prev_location; t.prev_noise = m.d_prev_noise;
    return t;
}
static int launch_scripted(mate_engine *e, const OpponentPlan &op, int freeze_done, hipStream_t stream) {
    ScriptedArgs a{};
    for (int team = 0; team < 2; ++team) a.team[team] = scripted_team_args(e, team, op.team[team].scripted);
    a.tape = e->scripted.tape; a.record = e->scripted.record; a.freeze_done = freeze_done;
    const Tiles tile = plan_attached_tile(e);
    HIP_TRY(launch_scripted_opponents(tile.blocks, tile.lds, stream, e->d_params, e->g, a));
    return MATE_OK;
}

// The agents' launch of the two-launch form with a channel in it: greedy_channel_kernel for the teams `q.caller_team` lets act.  Identical arguments at every
// call but for the team the caller plays, no allocation, no synchronisation.
static ChannelArgs channel_args(const mate_engine *e, const OpponentPlan &op) {
    ChannelArgs a{};
    for (int team = 0; team < 2; ++team) {
        const Channels::Team &c = e->channel.team[team];
        ChannelTeam &t = a.team[team];
        t.set = c.set; t.disabled = c.disabled; t.limit = c.limit; t.rate = c.rate; t.mask = c.mask;
        t.tape_u = c.tape_u; t.record_u = c.record_u; t.sent = c.d_sent; t.delivered = c.d_delivered;
        if (op.team[team].scripted) {
            const ScriptedMixture &m = e->scripted.team[team];
            t.mix.on = 1; t.mix.count = m.count;
            for (int i = 0; i < kScriptedKinds; ++i) { t.mix.kinds[i] = m.kinds[i]; t.mix.cum[i] = m.cum[i]; }
            t.mix.episode = m.d_episode; t.mix.choice = m.d_choice;
            t.mix.tape_choice = e->scripted.tape.choice ? e->scripted.tape.choice + (int64_t)team * e->N : nullptr;
        }
    }
    a.lds_bytes = e->channel.lds_bytes;
    return a;
}

// The Heuristic camera opponent (include/mate_engine.h, csrc/opponent_rows.hpp): tables, tapes, selection, goals.
extern "C" int mate_engine_heuristic_camera_tables(mate_engine *e, const double *state_mesh, const double *coord_grid, const double *scores) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (!state_mesh || !coord_grid || !scores) return fail(MATE_EINVAL, "heuristic_camera_tables: null table");
    MATE_TRY(enter_host(e));      // (no launch in flight reads the tables while they change)
    CameraOpponent &o = e->camera_opponent;
    if (!o.d_scores) {
        MATE_TRY(dev_alloc(e, &o.d_mesh, (size_t)kHcStates * 3, false));
        MATE_TRY(dev_alloc(e, &o.d_grid, (size_t)kHcPoints * 2, false));
        MATE_TRY(dev_alloc(e, &o.d_scores, (size_t)kHcPoints * kHcStates, false));
    }
    HIP_TRY(hipMemcpy(o.d_mesh, state_mesh, sizeof(double) * kHcStates * 3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(o.d_grid, coord_grid, sizeof(double) * kHcPoints * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(o.d_scores, scores, sizeof(double) * (size_t)kHcPoints * kHcStates, hipMemcpyHostToDevice));
    return MATE_OK;
}
extern "C" int mate_engine_heuristic_camera_tape(mate_engine *e, const int8_t *permutations_dev, int8_t *record_dev) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    MATE_TRY(enter_host(e));
    e->camera_opponent.permutations = permutations_dev; e->camera_opponent.record = record_dev;
    return MATE_OK;
}
extern "C" int mate_engine_heuristic_camera_goals(mate_engine *e, double *goals_dev, int32_t *indices_dev, void *stream) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    const CameraOpponent &o = e->camera_opponent;
    if (!o.d_goals) return fail(MATE_ESTATE, "heuristic_camera_goals: the heuristic camera opponent has not been selected (mate_engine_set_camera_opponent)");
    HIP_TRY(hipSetDevice(e->device));
    note_stream(e, (hipStream_t)stream);
    if (goals_dev) HIP_TRY(hipMemcpyAsync(goals_dev, o.d_goals, sizeof(double) * 2 * e->p.Nc * (size_t)e->N, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (indices_dev) HIP_TRY(hipMemcpyAsync(indices_dev, o.d_index, sizeof(int32_t) * e->p.Nc * (size_t)e->N, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MATE_OK;
}
// The Greedy agents of `team` run their agent.reset at their next acting call (PolCtx::cam_episode / tgt_episode <- -1): they sat out while a mixture's other
// candidates or the Heuristic cameras played.  The only writer of that mark.
static int mark_greedy_reset(mate_engine *e, int team) {
    unsigned char *episode = reinterpret_cast<unsigned char *>(e->q.pol) + pol_episode_offset(team == MATE_TEAM_CAMERA, e->p.Nc, e->p.Nt);
    HIP_TRY(hipMemset2D(episode, sizeof(double) * (size_t)e->q.PW, 0xff, sizeof(int32_t), (size_t)e->N));
    return MATE_OK;
}
// A Heuristic camera agent plays or could play the camera team with `kind` its plain selection and `m` its mixture.  Its fallback for a lost response is not on the
// device, so it and a channel of the camera team exclude each other: set_channel, set_camera_opponent and set_opponent_mixture each refuse whichever comes second.
static bool heuristic_camera_reachable(int kind, const ScriptedMixture &m) {
    return kind == MATE_OPPONENT_HEURISTIC || m.has[MATE_SCRIPTED_HEURISTIC] || (m.installed && m.restore == MATE_OPPONENT_HEURISTIC);
}
// Which scripted agent plays `team` where the engine plays it (include/mate_engine.h): the setters' and the mixture setter's one way to the plain selection.
// Targets: no agent memory differs between the two, so the switch is a flag and, once, the drift buffer.  Cameras: the Heuristic agents' memory, and the
// Greedy agents' reset when they come back.
static int set_plain_opponent(mate_engine *e, int team, int32_t opponent) {
    static const char *const needs[2] = {"the Greedy agents of the other team", "the Greedy agents the heuristic opponent builds on"};
    const char *name = kTeamNames[team];
    if (opponent != MATE_OPPONENT_GREEDY && opponent != MATE_OPPONENT_HEURISTIC) return fail(MATE_EINVAL, "set_%s_opponent: the opponent must be MATE_OPPONENT_GREEDY or MATE_OPPONENT_HEURISTIC", name);
    if (!e->policy_ready) return fail(MATE_ESTATE, "set_%s_opponent: call mate_engine_policy_enable() first (%s, and the engine's own view masks)", name, needs[team]);
    if (opponent == MATE_OPPONENT_HEURISTIC && e->team_mode[team] != 0)
        return fail(MATE_EINVAL, "set_%s_opponent: the heuristic %s opponent senses the %ss of its plain rows, the %s team's observation mode is %d (mate_engine_set_obs_mode)", name, name, kTeamNames[1 - team], name, e->team_mode[team]);
    CameraOpponent &o = e->camera_opponent;
    const int Nc = e->p.Nc;
    int &kind = e->opponents.kind[team];
    if (team == MATE_TEAM_CAMERA && opponent == MATE_OPPONENT_HEURISTIC && Nc > 0 && !o.d_scores)
        return fail(MATE_ESTATE, "set_camera_opponent: install the heuristic camera tables first (mate_engine_heuristic_camera_tables)");
    MATE_TRY(enter_host(e));      // (no launch in flight reads the buffers the getters switch between)
    if (team == MATE_TEAM_TARGET) {
        if (opponent == MATE_OPPONENT_HEURISTIC && !e->opponents.d_drift) MATE_TRY(dev_alloc(e, &e->opponents.d_drift, (size_t)e->N * e->p.Nt * 2));
        kind = opponent;
        return MATE_OK;
    }
    if (opponent == kind) return MATE_OK;
    if (Nc == 0) { kind = opponent; return MATE_OK; }      // (nobody to play: a no-op, OpponentPlan::Team::engine)
    if (opponent == MATE_OPPONENT_HEURISTIC) {
        if (!o.d_action) {
            const size_t pairs = (size_t)e->N * Nc * 2;
            MATE_TRY(dev_alloc(e, &o.d_prev, pairs));
            MATE_TRY(dev_alloc(e, &o.d_goals, pairs));
            MATE_TRY(dev_alloc(e, &o.d_index, (size_t)e->N * Nc));
            MATE_TRY(dev_alloc(e, &o.d_episode, (size_t)e->N));
            const hipError_t err = set_dynamic_lds(heuristic_camera_function(), heuristic_camera_lds_bytes(Nc));
            if (err != hipSuccess) return fail(MATE_EHIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(err));
            MATE_TRY(dev_alloc(e, &o.d_action, pairs));      // (last: its presence says all of the above is there)
        }
        // the agents start afresh: prev_action (0, 0), and their reset at the first acting call whatever the episode
        HIP_TRY(hipMemset(o.d_prev, 0, sizeof(double) * 2 * Nc * (size_t)e->N));
        HIP_TRY(hipMemset(o.d_episode, 0xff, sizeof(int32_t) * (size_t)e->N));
        o.ran = false;
    } else if (o.ran) MATE_TRY(mark_greedy_reset(e, MATE_TEAM_CAMERA));      // the Greedy camera agents sat out while the Heuristic ones played
    kind = opponent;
    return MATE_OK;
}
// While a learner's seat is enabled on `team` (mate_engine_enable_seat) its teammates stay plain Greedy agents without a channel: the setters ask here.
static int refuse_under_seat(const mate_engine *e, int team, const char *who, bool installs) {
    if (!installs || !e->seat.on || e->seat.spec.team != team) return MATE_OK;
    return fail(MATE_ESTATE, "%s: a learner's seat is enabled on the %s team (mate_engine_enable_seat), whose teammates are plain Greedy agents without a channel: disable the seat first", who, kTeamNames[team]);
}
static int refuse_under_mixture(const mate_engine *e, int team) {
    if (!e->scripted.team[team].installed) return MATE_OK;
    return fail(MATE_ESTATE, "set_%s_opponent: an opponent mixture is installed for the %s team (mate_engine_set_opponent_mixture): clear it first (count = 0)", kTeamNames[team], kTeamNames[team]);
}
extern "C" int mate_engine_set_camera_opponent(mate_engine *e, int32_t opponent) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    MATE_TRY(refuse_under_mixture(e, MATE_TEAM_CAMERA));
    MATE_TRY(refuse_under_seat(e, MATE_TEAM_CAMERA, "set_camera_opponent", opponent == MATE_OPPONENT_HEURISTIC));
    if (e->channel.team[MATE_TEAM_CAMERA].set && heuristic_camera_reachable(opponent, e->scripted.team[MATE_TEAM_CAMERA]))
        return fail(MATE_ESTATE, "set_camera_opponent: a communication channel is set for the camera team (mate_engine_set_channel), and the heuristic camera agent's fallback for a lost response is not on the device: clear the channel first");
    return set_plain_opponent(e, MATE_TEAM_CAMERA, opponent);
}
extern "C" int mate_engine_set_target_opponent(mate_engine *e, int32_t opponent) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    MATE_TRY(refuse_under_mixture(e, MATE_TEAM_TARGET));
    MATE_TRY(refuse_under_seat(e, MATE_TEAM_TARGET, "set_target_opponent", opponent == MATE_OPPONENT_HEURISTIC));
    return set_plain_opponent(e, MATE_TEAM_TARGET, opponent);
}

// The opponent mixtures (include/mate_engine.h, csrc/scripted_rows.hpp): install / clear, draws, memory, the external rows.
extern "C" int mate_engine_set_opponent_mixture(mate_engine *e, int32_t team, const int32_t *kinds, const double *weights, int32_t count, int32_t random_frame_skip) {
    const char *const *names = kTeamNames;
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (team != MATE_TEAM_CAMERA && team != MATE_TEAM_TARGET) return fail(MATE_EINVAL, "set_opponent_mixture: team must be MATE_TEAM_CAMERA or MATE_TEAM_TARGET");
    if (count < 0 || count > kScriptedKinds || (count > 0 && !kinds)) return fail(MATE_EINVAL, "set_opponent_mixture: the %s mixture takes 0 .. %d candidates (got %d) and their kinds", names[team], kScriptedKinds, count);
    // every check ahead of every change: a refused call leaves the engine as it was
    ScriptedMixture next;
    double total = 0.0;
    for (int i = 0; i < count; ++i) {
        const int kind = kinds[i];
        const double w = weights ? weights[i] : 1.0;
        if (kind < 0 || kind >= kScriptedKinds) return fail(MATE_EINVAL, "set_opponent_mixture: candidate %d of the %s mixture has the unknown kind %d (MATE_SCRIPTED_*)", i, names[team], kind);
        for (int k = 0; k < i; ++k) if (kinds[k] == kind) return fail(MATE_EINVAL, "set_opponent_mixture: kind %d appears twice in the %s mixture", kind, names[team]);
        if (!std::isfinite(w) || w < 0.0) return fail(MATE_EINVAL, "set_opponent_mixture: weight %d of the %s mixture is negative or not finite", i, names[team]);
        total += w;
    }
    if (count > 0 && !(total > 0.0)) return fail(MATE_EINVAL, "set_opponent_mixture: every weight of the %s mixture is zero", names[team]);
    if (random_frame_skip < 1) return fail(MATE_EINVAL, "set_opponent_mixture: random_frame_skip of the %s mixture must be at least 1 (got %d)", names[team], random_frame_skip);
    double running = 0.0;
    for (int i = 0; i < count; ++i) {      // the candidates with positive weight in the order given (mixture.py:41-43): p = w / sum, cum = cumsum(p)
        const double w = weights ? weights[i] : 1.0;
        if (!(w > 0.0)) continue;
        running += w / total;
        next.kinds[next.count] = kinds[i]; next.cum[next.count] = running; next.has[kinds[i]] = true; ++next.count;
    }
    if (!e->policy_ready) return fail(MATE_ESTATE, "set_opponent_mixture (%s team): call mate_engine_policy_enable() first (the Greedy agents, and the engine's own view masks)", names[team]);
    MATE_TRY(refuse_under_seat(e, team, "set_opponent_mixture", next.count > 0 && !(next.count == 1 && next.kinds[0] == MATE_SCRIPTED_GREEDY)));
    const int mode = e->team_mode[team];
    if (next.has[MATE_SCRIPTED_HEURISTIC] && mode != 0)
        return fail(MATE_EINVAL, "set_opponent_mixture: the Heuristic candidate of the %s mixture senses the opponents of its plain rows, the team's observation mode is %d (mate_engine_set_obs_mode)", names[team], mode);
    if (next.has[MATE_SCRIPTED_HEURISTIC] && team == MATE_TEAM_CAMERA && e->p.Nc > 0 && !e->camera_opponent.d_scores)
        return fail(MATE_ESTATE, "set_opponent_mixture: the camera mixture has a Heuristic candidate: install the heuristic camera tables first (mate_engine_heuristic_camera_tables)");
    if (team == MATE_TEAM_CAMERA && e->channel.team[MATE_TEAM_CAMERA].set && next.has[MATE_SCRIPTED_HEURISTIC])      // (heuristic_camera_reachable once `next` is installed: under a set channel the plain kind and the restore kind are Greedy)
        return fail(MATE_ESTATE, "set_opponent_mixture: the camera mixture has a Heuristic candidate and a communication channel is set for the camera team (mate_engine_set_channel): clear the channel first");
    MATE_TRY(enter_host(e));      // (no launch in flight reads what changes below)
    ScriptedMixture &m = e->scripted.team[team];
    const int n = agents_of(e, team);
    const int restore = m.installed ? m.restore : e->opponents.kind[team];
    if (count == 0) {                      // clear: the plain selection the mixture replaced; Greedy agents that sat out start afresh
        if (!m.installed) return MATE_OK;
        const bool launched = m.launch;
        MATE_TRY(set_plain_opponent(e, team, restore));
        m.installed = m.launch = false; m.count = 0;
        for (bool &h : m.has) h = false;
        return launched ? mark_greedy_reset(e, team) : MATE_OK;
    }
    next.launch = n > 0 && !(next.count == 1 && (next.kinds[0] == MATE_SCRIPTED_GREEDY || next.kinds[0] == MATE_SCRIPTED_HEURISTIC));
    if (next.launch && !m.d_final) {       // the memory of scripted_opponent_kernel, once
        const size_t pairs = (size_t)e->N * n * 2;
        MATE_TRY(dev_alloc(e, &m.d_external, pairs));
        MATE_TRY(dev_alloc(e, &m.d_prev_action, pairs));
        MATE_TRY(dev_alloc(e, &m.d_episode, (size_t)e->N));
        MATE_TRY(dev_alloc(e, &m.d_choice, (size_t)e->N));
        MATE_TRY(dev_alloc(e, &m.d_counter, (size_t)e->N));
        if (team == MATE_TEAM_TARGET) {
            MATE_TRY(dev_alloc(e, &m.d_prev_location, pairs));
            MATE_TRY(dev_alloc(e, &m.d_prev_noise, pairs));
            MATE_TRY(dev_alloc(e, &m.d_goal, (size_t)e->N * n));
            MATE_TRY(dev_alloc(e, &m.d_inc, (size_t)e->N * n));
        }
        MATE_TRY(dev_alloc(e, &m.d_final, pairs));      // (last: its presence says all of the above is there)
    }
    // the Heuristic machinery of the team is on exactly where a candidate needs it (plan_opponents reads the plain selection)
    MATE_TRY(set_plain_opponent(e, team, next.has[MATE_SCRIPTED_HEURISTIC] ? MATE_OPPONENT_HEURISTIC : MATE_OPPONENT_GREEDY));
    // Greedy agents that sat out under the old mixture and act under the new one (as a candidate, or as the plain selection) start afresh, as the
    // reference's new mixture agent resets the candidate it draws
    auto runs_greedy = [&](const ScriptedMixture &x) { return !x.launch || x.has[MATE_SCRIPTED_GREEDY] || (team == MATE_TEAM_TARGET && x.has[MATE_SCRIPTED_HEURISTIC]); };
    if (m.launch && !runs_greedy(m) && runs_greedy(next)) MATE_TRY(mark_greedy_reset(e, team));
    if (next.launch) {                     // the team's reset, the draw included, at its next acting call whatever the episode
        HIP_TRY(hipMemset(m.d_episode, 0xff, sizeof(int32_t) * (size_t)e->N));
        HIP_TRY(hipMemset(m.d_choice, 0xff, sizeof(int32_t) * (size_t)e->N));
    }
    m.installed = true; m.launch = next.launch; m.restore = restore; m.frame_skip = random_frame_skip;
    m.count = next.count;
    for (int i = 0; i < kScriptedKinds; ++i) { m.kinds[i] = next.kinds[i]; m.cum[i] = next.cum[i]; m.has[i] = next.has[i]; }
    return MATE_OK;
}
// The communication channels (include/mate_engine.h, csrc/channel_rows.hpp): settings, draws, edge matrices.
static int channel_buffers(mate_engine *e) {      // the edge matrices of both teams and the kernel's LDS, once
    Channels &c = e->channel;
    if (c.lds_bytes) return MATE_OK;
    const int lds = round_up(e->q.lds_bytes + channel_staging_bytes(e->p.Nc, e->p.Nt), 16);
    if (4 * (size_t)lds > kLdsCeiling) return fail(MATE_EINVAL, "set_channel: %zu bytes of LDS per workgroup do not fit", 4 * (size_t)lds);
    for (int team = 0; team < 2; ++team) {
        const size_t n = (size_t)agents_of(e, team);
        if (!c.team[team].d_sent) MATE_TRY(dev_alloc(e, &c.team[team].d_sent, (size_t)e->N * n * n));
        if (!c.team[team].d_delivered) MATE_TRY(dev_alloc(e, &c.team[team].d_delivered, (size_t)e->N * n * n));
    }
    for (int f64 = 0; f64 < 2; ++f64) {
        const hipError_t err = set_dynamic_lds(greedy_channel_function(f64 != 0), 4 * (size_t)lds);
        if (err != hipSuccess) return fail(MATE_EHIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(err));
    }
    c.lds_bytes = lds;
    return MATE_OK;
}
extern "C" int mate_engine_set_channel(mate_engine *e, int32_t team, const mate_channel *cfg) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (team != MATE_TEAM_CAMERA && team != MATE_TEAM_TARGET) return fail(MATE_EINVAL, "set_channel: team must be MATE_TEAM_CAMERA or MATE_TEAM_TARGET");
    if (cfg && (!std::isfinite(cfg->dropout_rate) || cfg->dropout_rate < 0.0 || cfg->dropout_rate > 1.0))
        return fail(MATE_EINVAL, "set_channel: the dropout rate must lie in [0, 1] (got %g)", cfg->dropout_rate);
    if (cfg && std::isnan(cfg->range_limit)) return fail(MATE_EINVAL, "set_channel: the range limit is NaN (negative or +inf: no limit)");
    if (!e->policy_ready) return fail(MATE_ESTATE, "set_channel: call mate_engine_policy_enable() first (the agents whose messages the channel carries)");
    MATE_TRY(refuse_under_seat(e, team, "set_channel", cfg != nullptr));
    if (cfg && team == MATE_TEAM_CAMERA && heuristic_camera_reachable(e->opponents.kind[MATE_TEAM_CAMERA], e->scripted.team[MATE_TEAM_CAMERA]))
            return fail(MATE_ESTATE, "set_channel: the heuristic camera agent plays (or is a candidate of) the camera team, and its fallback for a lost response is not on the device: select MATE_OPPONENT_GREEDY first");
    MATE_TRY(enter_host(e));      // (no launch in flight reads the settings)
    MATE_TRY(channel_buffers(e));
    Channels::Team &c = e->channel.team[team];
    if (!cfg) { c.set = false; c.disabled = false; c.limit = -1.0; c.rate = 0.0; c.mask = nullptr; return MATE_OK; }
    c.set = true; c.disabled = cfg->disabled != 0;
    c.limit = (cfg->range_limit < 0.0 || std::isinf(cfg->range_limit)) ? -1.0 : cfg->range_limit;
    c.rate = cfg->dropout_rate; c.mask = cfg->mask_dev;
    return MATE_OK;
}
extern "C" int mate_engine_channel_tape(mate_engine *e, const double *camera_u_dev, const double *target_u_dev, double *record_camera_u_dev, double *record_target_u_dev) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if ((reinterpret_cast<uintptr_t>(camera_u_dev) & 7u) || (reinterpret_cast<uintptr_t>(target_u_dev) & 7u) || (reinterpret_cast<uintptr_t>(record_camera_u_dev) & 7u) || (reinterpret_cast<uintptr_t>(record_target_u_dev) & 7u))
        return fail(MATE_EINVAL, "channel_tape: a buffer is not aligned to its element size");
    MATE_TRY(enter_host(e));
    e->channel.team[MATE_TEAM_CAMERA].tape_u = camera_u_dev; e->channel.team[MATE_TEAM_TARGET].tape_u = target_u_dev;
    e->channel.team[MATE_TEAM_CAMERA].record_u = record_camera_u_dev; e->channel.team[MATE_TEAM_TARGET].record_u = record_target_u_dev;
    return MATE_OK;
}
extern "C" int mate_engine_channel_edges(mate_engine *e, int32_t team, int8_t **sent_dev, int8_t **delivered_dev) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (team != MATE_TEAM_CAMERA && team != MATE_TEAM_TARGET) return fail(MATE_EINVAL, "channel_edges: team must be MATE_TEAM_CAMERA or MATE_TEAM_TARGET");
    if (!e->policy_ready) return fail(MATE_ESTATE, "channel_edges: call mate_engine_policy_enable() first");
    if (!e->channel.lds_bytes) {
        MATE_TRY(enter_host(e));
        MATE_TRY(channel_buffers(e));
    }
    if (sent_dev) *sent_dev = e->channel.team[team].d_sent;
    if (delivered_dev) *delivered_dev = e->channel.team[team].d_delivered;
    return MATE_OK;
}
extern "C" int mate_engine_scripted_tape(mate_engine *e, const double *camera_u_dev, const double *target_u_dev, const double *target_reset_dev, const int32_t *choice_dev,
                                         double *record_camera_u_dev, double *record_target_u_dev, double *record_target_reset_dev, int32_t *record_choice_dev) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if ((reinterpret_cast<uintptr_t>(record_camera_u_dev) & 15u) || (reinterpret_cast<uintptr_t>(record_target_reset_dev) & 15u))
        return fail(MATE_EINVAL, "scripted_tape: record_camera_u_dev and record_target_reset_dev must be aligned to 16 bytes (the launch stores pairs of doubles)");
    if ((reinterpret_cast<uintptr_t>(camera_u_dev) & 7u) || (reinterpret_cast<uintptr_t>(target_u_dev) & 7u) || (reinterpret_cast<uintptr_t>(target_reset_dev) & 7u) ||
        (reinterpret_cast<uintptr_t>(record_target_u_dev) & 7u) || (reinterpret_cast<uintptr_t>(choice_dev) & 3u) || (reinterpret_cast<uintptr_t>(record_choice_dev) & 3u))
        return fail(MATE_EINVAL, "scripted_tape: a buffer is not aligned to its element size");
    MATE_TRY(enter_host(e));
    // (ScriptedDraws is one type for both: the launch only ever reads through `tape`)
    e->scripted.tape = ScriptedDraws{const_cast<double *>(camera_u_dev), const_cast<double *>(target_u_dev), const_cast<double *>(target_reset_dev), const_cast<int32_t *>(choice_dev)};
    e->scripted.record = ScriptedDraws{record_camera_u_dev, record_target_u_dev, record_target_reset_dev, record_choice_dev};
    return MATE_OK;
}
extern "C" int mate_engine_scripted_memory(mate_engine *e, int32_t team, int32_t *choice_dev, int32_t *goal_dev, int32_t *inc_dev, double *prev_noise_dev, double *prev_action_dev,
                                           int32_t *counter_dev, void *stream_) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (team != MATE_TEAM_CAMERA && team != MATE_TEAM_TARGET) return fail(MATE_EINVAL, "scripted_memory: team must be MATE_TEAM_CAMERA or MATE_TEAM_TARGET");
    const ScriptedMixture &m = e->scripted.team[team];
    if (!m.d_final) return fail(MATE_ESTATE, "scripted_memory: no opponent mixture with a launch of its own has been installed for the team (mate_engine_set_opponent_mixture)");
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(e->device));
    note_stream(e, stream);
    const size_t N = (size_t)e->N, n = (size_t)agents_of(e, team);
    if (choice_dev) HIP_TRY(hipMemcpyAsync(choice_dev, m.d_choice, sizeof(int32_t) * N, hipMemcpyDeviceToDevice, stream));
    if (counter_dev) HIP_TRY(hipMemcpyAsync(counter_dev, m.d_counter, sizeof(int32_t) * N, hipMemcpyDeviceToDevice, stream));
    if (prev_action_dev) HIP_TRY(hipMemcpyAsync(prev_action_dev, m.d_prev_action, sizeof(double) * 2 * n * N, hipMemcpyDeviceToDevice, stream));
    if (team == MATE_TEAM_TARGET) {
        if (goal_dev) HIP_TRY(hipMemcpyAsync(goal_dev, m.d_goal, sizeof(int32_t) * n * N, hipMemcpyDeviceToDevice, stream));
        if (inc_dev) HIP_TRY(hipMemcpyAsync(inc_dev, m.d_inc, sizeof(int32_t) * n * N, hipMemcpyDeviceToDevice, stream));
        if (prev_noise_dev) HIP_TRY(hipMemcpyAsync(prev_noise_dev, m.d_prev_noise, sizeof(double) * 2 * n * N, hipMemcpyDeviceToDevice, stream));
    }
    return MATE_OK;
}
extern "C" int mate_engine_scripted_external(mate_engine *e, int32_t team, double **rows_dev) {
    if (!e || !rows_dev) return fail(MATE_EINVAL, "null argument");
    if (team != MATE_TEAM_CAMERA && team != MATE_TEAM_TARGET) return fail(MATE_EINVAL, "scripted_external: team must be MATE_TEAM_CAMERA or MATE_TEAM_TARGET");
    if (!e->scripted.team[team].d_final) return fail(MATE_ESTATE, "scripted_external: no opponent mixture with a launch of its own has been installed for the team (mate_engine_set_opponent_mixture)");
    *rows_dev = e->scripted.team[team].d_external;
    return MATE_OK;
}
extern "C" int mate_engine_scripted_rows(mate_engine *e, int32_t team, int32_t kind, double *rows_dev, void *stream) {
    if (!e || !rows_dev) return fail(MATE_EINVAL, "null argument");
    if (team != MATE_TEAM_CAMERA && team != MATE_TEAM_TARGET) return fail(MATE_EINVAL, "scripted_rows: team must be MATE_TEAM_CAMERA or MATE_TEAM_TARGET");
    if (kind != MATE_SCRIPTED_GREEDY && kind != MATE_SCRIPTED_HEURISTIC && kind != MATE_SCRIPTED_EXTERNAL)
        return fail(MATE_EINVAL, "scripted_rows: the sources are MATE_SCRIPTED_GREEDY, _HEURISTIC and _EXTERNAL (the Naive and Random rows exist as final rows only)");
    if (!e->policy_ready) return fail(MATE_ESTATE, "scripted_rows: policies are not enabled");
    const double *src = kind == MATE_SCRIPTED_EXTERNAL ? e->scripted.team[team].d_external : rows_of(e, team, kind == MATE_SCRIPTED_GREEDY ? ROWS_GREEDY : ROWS_HEURISTIC);
    if (!src || (kind == MATE_SCRIPTED_HEURISTIC && !e->scripted.team[team].has[MATE_SCRIPTED_HEURISTIC]))
        return fail(MATE_ESTATE, "scripted_rows: the team's mixture (mate_engine_set_opponent_mixture) has no such source");
    HIP_TRY(hipSetDevice(e->device));
    note_stream(e, (hipStream_t)stream);
    HIP_TRY(hipMemcpyAsync(rows_dev, src, sizeof(double) * 2 * (size_t)agents_of(e, team) * (size_t)e->N, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MATE_OK;
}

// The learner's seat among on-device teammates (include/mate_engine.h, csrc/seat_rows.hpp): enable / change / disable, the launches' arguments.
static const char *seat_refusal_text(int refusal) {
    switch (refusal) {
    case SEAT_HEURISTIC: return "the team's plain selection is the Heuristic agent (mate_engine_set_camera_opponent / _set_target_opponent): select MATE_OPPONENT_GREEDY first";
    case SEAT_MIXTURE: return "the team plays an opponent mixture other than {Greedy} (mate_engine_set_opponent_mixture): clear it first";
    case SEAT_CHANNEL: return "a communication channel is set for the team (mate_engine_set_channel): clear it first";
    case SEAT_OPPOSING_CHANNEL: return "the opposing team's communication channel is live (mate_engine_set_channel), and its agents' launch is greedy_channel_kernel: clear it first";
    default: return "";
    }
}
extern "C" int mate_engine_enable_seat(mate_engine *e, int32_t team, int32_t mode, int32_t fixed_seat, const int32_t *seat_tape_dev, void *obs_out_dev, int32_t *seat_index_dev, int32_t *seat_acted_dev) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    Seat &s = e->seat;
    if (!obs_out_dev && !seat_index_dev && !seat_acted_dev) {      // the disable form: the team's Greedy agents start afresh at their next acting call
        if (!s.on) return MATE_OK;
        MATE_TRY(enter_host(e));
        MATE_TRY(mark_greedy_reset(e, s.spec.team));
        s.on = false;
        return MATE_OK;
    }
    if (team != MATE_TEAM_CAMERA && team != MATE_TEAM_TARGET) return fail(MATE_EINVAL, "enable_seat: team must be MATE_TEAM_CAMERA or MATE_TEAM_TARGET");
    const int n = agents_of(e, team);
    if (n == 0) return fail(MATE_EINVAL, "enable_seat: the scenario has no %ss to sit among", kTeamNames[team]);
    if (mode != MATE_SEAT_FIXED && mode != MATE_SEAT_DRAW && mode != MATE_SEAT_TAPE) return fail(MATE_EINVAL, "enable_seat: mode must be MATE_SEAT_FIXED, MATE_SEAT_DRAW or MATE_SEAT_TAPE");
    if (mode == MATE_SEAT_FIXED && fixed_seat < 0) fixed_seat = n - 1;      // (the wrapper's index with shuffle_entities off)
    if (mode == MATE_SEAT_FIXED && fixed_seat >= n) return fail(MATE_EINVAL, "enable_seat: the fixed seat %d is outside [0, %d)", fixed_seat, n);
    if (mode == MATE_SEAT_TAPE && !seat_tape_dev) return fail(MATE_EINVAL, "enable_seat: MATE_SEAT_TAPE needs seat_tape_dev");
    if (!obs_out_dev || !seat_index_dev || !seat_acted_dev) return fail(MATE_EINVAL, "enable_seat: obs_out_dev, seat_index_dev and seat_acted_dev must all be there (all three NULL: disable)");
    if ((reinterpret_cast<uintptr_t>(obs_out_dev) & 15u) || ((reinterpret_cast<uintptr_t>(seat_index_dev) | reinterpret_cast<uintptr_t>(seat_acted_dev) | reinterpret_cast<uintptr_t>(seat_tape_dev)) & 3u))
        return fail(MATE_EINVAL, "enable_seat: obs_out_dev must be 16-byte aligned, the int32 buffers aligned to their element size");
    if (!e->policy_ready) return fail(MATE_ESTATE, "enable_seat: call mate_engine_policy_enable() first (the teammates, and the engine's own view masks)");
    if (s.on && s.spec.team != team) return fail(MATE_ESTATE, "enable_seat: a seat is enabled on the %s team, and an engine has one seat team: disable it first", kTeamNames[s.spec.team]);
    const OpponentPlan op = plan_opponents(e, -1, team);
    if (op.seat_refusal != SEAT_OK) return fail(MATE_ESTATE, "enable_seat (%s team): %s", kTeamNames[team], seat_refusal_text(op.seat_refusal));
    MATE_TRY(enter_host(e));      // (no launch in flight reads what changes below)
    if (!s.d_live) MATE_TRY(dev_alloc(e, &s.d_live, (size_t)e->N));
    for (int f64 = 0; f64 < 2; ++f64) {
        const hipError_t err = set_dynamic_lds(greedy_seat_function(f64 != 0), 4 * (size_t)e->q.lds_bytes);
        if (err != hipSuccess) return fail(MATE_EHIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(err));
    }
    MATE_TRY(mark_greedy_reset(e, team));      // enabling or changing the seat: the team's agents run their reset at their next acting call (the mixtures' rule)
    s.spec = SeatSpec{team, mode, mode == MATE_SEAT_FIXED ? fixed_seat : 0, n, mode == MATE_SEAT_TAPE ? seat_tape_dev : nullptr};
    s.obs = obs_out_dev; s.index = seat_index_dev; s.acted = seat_acted_dev;
    s.on = true;
    return MATE_OK;
}
// Behind everything else of a seat call (`live`: the call's agents' launch ran; else on demand: every environment is written)
static int seat_rows_behind(mate_engine *e, const mate_step_io *io, bool live, hipStream_t stream) {
    const Seat &s = e->seat;
    const bool camera = s.spec.team == MATE_TEAM_CAMERA;
    const SeatRowsArgs a{s.spec, camera ? io->camera_obs_dev : io->target_obs_dev, s.obs, s.index, live ? s.d_live : nullptr, camera ? e->p.Dc : e->p.Dt};
    HIP_TRY(launch_seat_rows(e->p.obs_f64 != 0, blocks_of(e, kSeatRowsEnvs), stream, e->d_params, e->g, a));
    return MATE_OK;
}
