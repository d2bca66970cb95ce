// trace_host.inc -- the host side of the communication trace (include/mate_engine.h, csrc/trace_rows.hpp), included by mate_engine.hip behind render_host.inc
// (which it shares fail, HIP_TRY, MATE_TRY, dev_alloc, enter, enter_host, note_stream and agents_of with).  Host only: enable / detach, the one launch of a
// stepping call, the accessor, planting a caller's matrix.

extern "C" int mate_engine_enable_comm_trace(mate_engine *e, int32_t teams_mask, int32_t duration) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (teams_mask < 0 || teams_mask > 3) return fail(MATE_EINVAL, "enable_comm_trace: teams_mask is 0 (detach), 1 << MATE_TEAM_CAMERA, 1 << MATE_TEAM_TARGET or both (got %d)", teams_mask);
    if (teams_mask != 0) {
        if (duration < 1 || duration > 255) return fail(MATE_EINVAL, "enable_comm_trace: duration must lie in [1, 255] (got %d)", duration);
        for (int team = 0; team < 2; ++team)
            if (((teams_mask >> team) & 1) && agents_of(e, team) == 0) return fail(MATE_EINVAL, "enable_comm_trace: the scenario has no %ss to talk", kTeamNames[team]);
    }
    MATE_TRY(enter_host(e));                   // (no launch in flight reads what changes below; a pipelined-restart mode is left, as by every attachment)
    for (int team = 0; team < 2; ++team) {
        CommTrace::Team &t = e->trace.team[team];
        if (!((teams_mask >> team) & 1)) continue;
        const size_t n = (size_t)agents_of(e, team);
        if (!t.d_remaining) MATE_TRY(dev_alloc(e, &t.d_remaining, (size_t)e->N * n * n));      // (each pointer on its own: a failed second allocation leaks nothing at the next enable)
        if (!t.d_tags) MATE_TRY(dev_alloc(e, &t.d_tags, (size_t)e->N));
    }
    for (int team = 0; team < 2; ++team) e->trace.team[team].on = (teams_mask >> team) & 1;      // (behind every allocation: a refused call changes nothing)
    e->trace.duration = teams_mask ? duration : 0;
    for (int team = 0; team < 2; ++team) {     // an enabled team starts from zeros, tagged with no episode
        const CommTrace::Team &t = e->trace.team[team];
        const size_t n = (size_t)agents_of(e, team);
        if (!t.on) continue;
        HIP_TRY(hipMemset(t.d_tags, 0xff, sizeof(int32_t) * (size_t)e->N));
        HIP_TRY(hipMemset(t.d_remaining, 0, (size_t)e->N * n * n));
    }
    return MATE_OK;
}

extern "C" int mate_engine_comm_trace(mate_engine *e, int32_t team, uint8_t **remaining_dev, int32_t **tag_dev) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (team != MATE_TEAM_CAMERA && team != MATE_TEAM_TARGET) return fail(MATE_EINVAL, "comm_trace: team must be MATE_TEAM_CAMERA or MATE_TEAM_TARGET");
    const CommTrace::Team &t = e->trace.team[team];
    if (!t.on) return fail(MATE_ESTATE, "comm_trace: mate_engine_enable_comm_trace() has not enabled the %s team", kTeamNames[team]);
    if (remaining_dev) *remaining_dev = t.d_remaining;
    if (tag_dev) *tag_dev = t.d_tags;
    return MATE_OK;
}

// The caller's [N][n][n] matrix into the engine-owned one, tagged with the environments' episode numbers as they are: what render() then draws
extern "C" int mate_engine_set_comm_trace(mate_engine *e, int32_t team, const uint8_t *remaining_dev) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (team != MATE_TEAM_CAMERA && team != MATE_TEAM_TARGET) return fail(MATE_EINVAL, "set_comm_trace: team must be MATE_TEAM_CAMERA or MATE_TEAM_TARGET");
    if (!remaining_dev) return fail(MATE_EINVAL, "set_comm_trace: null matrix");
    const CommTrace::Team &t = e->trace.team[team];
    if (!t.on) return fail(MATE_ESTATE, "set_comm_trace: mate_engine_enable_comm_trace() has not enabled the %s team", kTeamNames[team]);
    if (!e->was_reset) return fail(MATE_ESTATE, "set_comm_trace called before reset() (or import_state)");
    MATE_TRY(enter_host(e));                   // (the caller's matrix is complete, no launch in flight reads the engine's)
    const int n = agents_of(e, team);
    HIP_TRY(launch_trace_plant(blocks_of(e, kAttachedEnvsPerBlock), e->last_stream, e->d_params, e->g.dyn, remaining_dev, t.d_remaining, t.d_tags, e->N, n * n));
    note_stream(e, e->last_stream);
    HIP_TRY(wait_for_launches(e));             // (complete when the call returns: the caller may free its matrix)
    return MATE_OK;
}

// 2d of AttachedPlan's order: the one launch of a stepping call, for the teams with a trace.  `freeze_done`: of the call
static int launch_trace(mate_engine *e, int freeze_done, hipStream_t stream) {
    if (!e->trace.on()) return MATE_OK;
    TraceArgs a{};
    for (int team = 0; team < 2; ++team) {
        const CommTrace::Team &t = e->trace.team[team];
        if (!t.on) continue;
        TraceTeam &out = a.team[team];
        out.n = agents_of(e, team); out.remaining = t.d_remaining; out.tags = t.d_tags;
        if (t.call_delivered) out.delivered = e->channel.team[team].d_delivered;
        const Messages::Team &m = e->messages.team[team];
        if (m.on) { out.step_edges = m.d_step; out.message_tags = m.d_tags; }
    }
    a.dyn = e->g.dyn; a.N = e->N; a.duration = e->trace.duration; a.freeze_done = freeze_done;
    HIP_TRY(launch_comm_trace(blocks_of(e, kAttachedEnvsPerBlock), stream, e->d_params, a));
    return MATE_OK;
}
