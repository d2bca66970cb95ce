// message_host.inc -- the host side of the learner's own messages (include/mate_engine.h, csrc/message_rows.hpp), included by mate_engine.hip behind
// opponent_host.inc (which it shares fail, HIP_TRY, MATE_TRY, dev_alloc, enter, enter_host and agents_of with).  Host only: enable / disable, the one launch,
// the draws, the accessors.  The router reads the environments' records and the team's channel settings, nothing of the on-device agents: it needs
// mate_engine_policy_enable only through mate_engine_set_channel, which does.

constexpr int kMessageWidthMax = 65536;      // numbers per message: n n width stays far inside 32-bit index arithmetic

extern "C" int mate_engine_enable_messages(mate_engine *e, int32_t team, const mate_message_rows *cfg) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (team != MATE_TEAM_CAMERA && team != MATE_TEAM_TARGET) return fail(MATE_EINVAL, "enable_messages: team must be MATE_TEAM_CAMERA or MATE_TEAM_TARGET");
    Messages::Team &m = e->messages.team[team];
    if (!cfg) {                                // the disable form: the buffers stay the engine's, the counts start afresh at the next enable
        if (!m.on) return MATE_OK;
        MATE_TRY(enter_host(e));
        m.on = false; m.payload = nullptr; m.address = nullptr; m.inbox = nullptr;
        return MATE_OK;
    }
    const size_t n = (size_t)agents_of(e, team);
    if (n == 0) return fail(MATE_EINVAL, "enable_messages: the scenario has no %ss to talk", kTeamNames[team]);
    if (cfg->width < 1 || cfg->width > kMessageWidthMax) return fail(MATE_EINVAL, "enable_messages: width must lie in [1, %d] (got %d)", kMessageWidthMax, cfg->width);
    if (!cfg->payload_dev || !cfg->inbox_dev) return fail(MATE_EINVAL, "enable_messages: payload_dev and inbox_dev must be there (a NULL cfg disables)");
    if ((reinterpret_cast<uintptr_t>(cfg->payload_dev) | reinterpret_cast<uintptr_t>(cfg->inbox_dev)) & 15u)
        return fail(MATE_EINVAL, "enable_messages: payload_dev and inbox_dev must be 16-byte aligned");
    MATE_TRY(enter_host(e));                   // (no launch in flight reads what changes below)
    if (!m.d_tags) {
        const size_t pairs = (size_t)e->N * n * n;
        MATE_TRY(dev_alloc(e, &m.d_sent, pairs));
        MATE_TRY(dev_alloc(e, &m.d_delivered, pairs));
        MATE_TRY(dev_alloc(e, &m.d_step, pairs));
        MATE_TRY(dev_alloc(e, &m.d_total, pairs));
        MATE_TRY(dev_alloc(e, &m.d_agent, (size_t)e->N * n * 2));
        MATE_TRY(dev_alloc(e, &m.d_tags, (size_t)e->N * 2));      // (last: its presence says all of the above is there)
    }
    HIP_TRY(hipMemset(m.d_tags, 0xff, sizeof(int32_t) * 2 * (size_t)e->N));      // no (tick, episode): the first launch zeroes the counts
    m.width = cfg->width; m.pairwise = cfg->pairwise != 0;
    m.payload = cfg->payload_dev; m.address = cfg->address_dev; m.inbox = cfg->inbox_dev;
    m.on = true;
    return MATE_OK;
}

// The launch's arguments: the teams of `team_mask`, each with its channel's settings as they are now
static MessageArgs message_args(const mate_engine *e, int32_t team_mask, int32_t round) {
    MessageArgs a{};
    for (int team = 0; team < 2; ++team) {
        if (!((team_mask >> team) & 1)) continue;
        const Messages::Team &m = e->messages.team[team];
        const Channels::Team &c = e->channel.team[team];
        MessageTeam &t = a.team[team];
        t.on = 1; t.n = agents_of(e, team); t.width = m.width; t.pairwise = m.pairwise;
        t.set = c.set; t.disabled = c.disabled; t.limit = c.limit; t.rate = c.rate; t.mask = c.mask;
        t.address = m.address; t.payload = m.payload; t.inbox = m.inbox;
        t.tape_u = m.tape_u; t.record_u = m.record_u;
        t.sent = m.d_sent; t.delivered = m.d_delivered;
        t.step_edges = m.d_step; t.total_edges = m.d_total; t.agent_edges = m.d_agent; t.tags = m.d_tags;
    }
    a.round = round;
    return a;
}
// Identical arguments at every call, no allocation, no synchronisation: capturable under mate_engine_device_tick.
extern "C" int mate_engine_route_messages(mate_engine *e, int32_t team_mask, int32_t round, void *stream) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (team_mask < 1 || team_mask > 3) return fail(MATE_EINVAL, "route_messages: team_mask is 1 << MATE_TEAM_CAMERA, 1 << MATE_TEAM_TARGET or both (got %d)", team_mask);
    if (round < 0 || round >= kMessageRounds) return fail(MATE_EINVAL, "route_messages: round must lie in [0, %d) (got %d)", kMessageRounds, round);
    for (int team = 0; team < 2; ++team)
        if (((team_mask >> team) & 1) && !e->messages.team[team].on)
            return fail(MATE_ESTATE, "route_messages: call mate_engine_enable_messages() for the %s team first", kTeamNames[team]);
    MATE_TRY(enter(e, (hipStream_t)stream, "route_messages"));
    note_stream(e, (hipStream_t)stream);
    HIP_TRY(launch_message_rows(e->p.obs_f64 != 0, blocks_of(e, 4), (hipStream_t)stream, e->d_params, e->g, message_args(e, team_mask, round)));
    return MATE_OK;
}

extern "C" int mate_engine_message_edges(mate_engine *e, int32_t team, int8_t **sent_dev, int8_t **delivered_dev, int32_t **step_edges_dev, int32_t **total_edges_dev, int32_t **agent_edges_dev) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (team != MATE_TEAM_CAMERA && team != MATE_TEAM_TARGET) return fail(MATE_EINVAL, "message_edges: team must be MATE_TEAM_CAMERA or MATE_TEAM_TARGET");
    const Messages::Team &m = e->messages.team[team];
    if (!m.d_tags) return fail(MATE_ESTATE, "message_edges: mate_engine_enable_messages() has not run for the %s team", kTeamNames[team]);
    if (sent_dev) *sent_dev = m.d_sent;
    if (delivered_dev) *delivered_dev = m.d_delivered;
    if (step_edges_dev) *step_edges_dev = m.d_step;
    if (total_edges_dev) *total_edges_dev = m.d_total;
    if (agent_edges_dev) *agent_edges_dev = m.d_agent;
    return MATE_OK;
}

extern "C" int mate_engine_message_tape(mate_engine *e, const double *camera_u_dev, const double *target_u_dev, double *record_camera_u_dev, double *record_target_u_dev) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if ((reinterpret_cast<uintptr_t>(camera_u_dev) | reinterpret_cast<uintptr_t>(target_u_dev) | reinterpret_cast<uintptr_t>(record_camera_u_dev) | reinterpret_cast<uintptr_t>(record_target_u_dev)) & 7u)
        return fail(MATE_EINVAL, "message_tape: a buffer is not aligned to its element size");
    MATE_TRY(enter_host(e));
    e->messages.team[MATE_TEAM_CAMERA].tape_u = camera_u_dev; e->messages.team[MATE_TEAM_TARGET].tape_u = target_u_dev;
    e->messages.team[MATE_TEAM_CAMERA].record_u = record_camera_u_dev; e->messages.team[MATE_TEAM_TARGET].record_u = record_target_u_dev;
    return MATE_OK;
}
