// frame_host.inc -- the host side of the per-frame FrameSkip fragments (include/mate_engine.h, csrc/frame_rows.hpp), included by mate_engine.hip behind
// message_host.inc (which it shares fail, HIP_TRY, MATE_TRY, enter, enter_host and agents_of with).  Host only: enable / disable, the check a stepping call of
// the attached team makes, the on-demand launch.  The launches of a call are in mate_engine.hip's attached section (launch_frame_of_call,
// launch_frame_first_rows), at the positions AttachedPlan gives them.

// Validates `cfg` and fills the launch's arguments but the call's own (the reward rows a shaped sum reads must be attached now)
static int frame_args_of(const mate_engine *e, const mate_frame_fragments *cfg, FrameArgs *out) {
    const Params &p = e->p;
    if (cfg->team != MATE_TEAM_CAMERA && cfg->team != MATE_TEAM_TARGET) return fail(MATE_EINVAL, "frame fragments: team must be MATE_TEAM_CAMERA or MATE_TEAM_TARGET");
    const bool camera = cfg->team == MATE_TEAM_CAMERA;
    if (camera && p.Nc == 0) return fail(MATE_EINVAL, "frame fragments: the scenario has no cameras to learn for");
    if (cfg->frames < 1) return fail(MATE_EINVAL, "frame fragments: frames must be at least 1 (got %d)", cfg->frames);
    const bool f64 = cfg->out_dtype == MATE_OBS_F64;
    if (cfg->out_dtype != MATE_OBS_F32 && !f64) return fail(MATE_EINVAL, "frame fragments: out_dtype must be MATE_OBS_F32 or MATE_OBS_F64");
    if (cfg->info_dev && !cfg->frames_dev) return fail(MATE_EINVAL, "frame fragments: info_dev needs frames_dev (the means divide by it)");
    if (cfg->first_rows && !cfg->obs_dev) return fail(MATE_EINVAL, "frame fragments: first_rows without obs_dev");
    if (cfg->final_obs_dev && cfg->final_obs_dev == cfg->obs_dev) return fail(MATE_EINVAL, "frame fragments: obs_dev and final_obs_dev must be two buffers");
    const int A = camera ? p.Nc : p.Nt, D = camera ? p.Dc : p.Dt;
    const uintptr_t obs_size = p.obs_f64 ? 8u : 4u;
    const uintptr_t row_align = obs_size - 1u;      // (the kernel takes 16-byte accesses where the row and the pointers allow them)
    auto misaligned = [](const void *ptr, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(ptr) & mask) != 0; };
    if (misaligned(cfg->obs_dev, row_align) || misaligned(cfg->final_obs_dev, row_align) || misaligned(cfg->rewards_dev, 7u) || misaligned(cfg->info_dev, 7u) ||
        misaligned(cfg->frames_dev, 3u) || misaligned(cfg->shaped_dev, f64 ? 7u : 3u))
        return fail(MATE_EINVAL, "frame fragments: a buffer is not aligned to its element size");
    if (cfg->shaped_dev) {
        const RewardRows &r = e->reward;
        if (!r.on || r.accumulate || !(camera ? r.args.cam_rows : r.args.tgt_rows))
            return fail(MATE_ESTATE, "frame fragments: shaped_dev sums the %s team's reward rows of every frame: attach them in overwrite mode first (mate_engine_enable_reward_rows)", kTeamNames[cfg->team]);
        if (r.f64 != f64) return fail(MATE_EINVAL, "frame fragments: shaped_dev is of another out_dtype than the attached reward rows");
    }
    FrameArgs a{};
    a.obs = cfg->obs_dev; a.final_obs = cfg->final_obs_dev; a.restarted = cfg->restarted_dev;
    a.rewards = cfg->rewards_dev; a.info = cfg->info_dev; a.done = cfg->done_dev; a.frames = cfg->frames_dev; a.shaped = cfg->shaped_dev;
    a.N = e->N; a.K = cfg->frames; a.A = A; a.D = D; a.shaped_f64 = f64;
    *out = a;
    return MATE_OK;
}

extern "C" int mate_engine_enable_frame_fragments(mate_engine *e, const mate_frame_fragments *cfg) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (!cfg) { e->frames = FrameFragments{}; return MATE_OK; }
    if (!e->was_reset) return fail(MATE_ESTATE, "enable_frame_fragments called before reset() (or import_state)");
    FrameArgs a;
    MATE_TRY(frame_args_of(e, cfg, &a));
    if (e->steps_since_reset != 0) return fail(MATE_ESTATE, "enable_frame_fragments inside an open restart interval (%lld calls in): the phase counts from the interval's first call", (long long)e->steps_since_reset);
    MATE_TRY(enter_host(e));                   // (leaves the pipelined-restart mode; no launch in flight reads what changes below)
    FrameFragments f;
    f.on = true; f.first_rows = cfg->first_rows != 0; f.team = cfg->team; f.args = a;
    e->frames = f;
    return MATE_OK;
}

// What a mate_engine_step_versus_greedy call of the attached team must bring, ahead of everything it enqueues
static int check_frame_call(const mate_engine *e, const mate_step_io *io, int auto_reset) {
    const FrameFragments &f = e->frames;
    const int K = f.args.K;
    if (auto_reset < 1 || auto_reset % K != 0)
        return fail(MATE_EINVAL, "per-frame fragments of %d frames are attached (mate_engine_enable_frame_fragments): auto_reset must be a positive multiple of %d (got %d)", K, K, auto_reset);
    const void *rows = io ? (f.team == MATE_TEAM_CAMERA ? io->camera_obs_dev : io->target_obs_dev) : nullptr;
    if (!io || !io->scalars_dev || (reinterpret_cast<uintptr_t>(io->scalars_dev) & 15u) || !rows)
        return fail(MATE_EINVAL, "per-frame fragments are attached (mate_engine_enable_frame_fragments): the call needs io->scalars_dev, 16-byte aligned, and the %s team's observation rows", kTeamNames[f.team]);
    if (f.args.obs && (rows == f.args.obs || rows == f.args.final_obs))
        return fail(MATE_EINVAL, "per-frame fragments: the call's observation rows and the fragment's obs_dev / final_obs_dev must be different buffers");
    if (e->steps_since_reset > 0 && e->pending_interval != (auto_reset | kStepFlow))
        return fail(MATE_ESTATE, "per-frame fragments are attached: auto_reset changed inside an open restart interval (the phase counts its calls)");
    if (f.args.shaped) {
        const RewardRows &r = e->reward;
        const bool camera = f.team == MATE_TEAM_CAMERA;
        if (!r.on || r.accumulate || !(camera ? r.args.cam_rows : r.args.tgt_rows) || r.f64 != (f.args.shaped_f64 != 0))
            return fail(MATE_ESTATE, "per-frame fragments with shaped_dev: the %s team's reward rows must stay attached in overwrite mode with the same out_dtype (mate_engine_enable_reward_rows)", kTeamNames[f.team]);
    }
    return MATE_OK;
}

// Identical arguments at every call, no allocation, no synchronisation
extern "C" int mate_engine_frame_fragment(mate_engine *e, const mate_frame_fragments *cfg, const mate_step_io *rows, int32_t phase, int32_t closes, void *stream) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (!cfg || !rows) return fail(MATE_EINVAL, "frame_fragment: null config or buffers");
    if (!e->was_reset) return fail(MATE_ESTATE, "frame_fragment called before reset() (or import_state)");
    FrameArgs a;
    MATE_TRY(frame_args_of(e, cfg, &a));
    if (phase < 0 || phase >= a.K) return fail(MATE_EINVAL, "frame_fragment: phase must lie in [0, %d) (got %d)", a.K, phase);
    if (closes != 0 && closes != 1) return fail(MATE_EINVAL, "frame_fragment: closes is 0 (the frame) or 1 (the first rows behind a restart)");
    const bool camera = cfg->team == MATE_TEAM_CAMERA;
    a.scalars = rows->scalars_dev;
    a.rows = camera ? rows->camera_obs_dev : rows->target_obs_dev;
    if (!a.scalars || (reinterpret_cast<uintptr_t>(a.scalars) & 15u)) return fail(MATE_EINVAL, "frame_fragment: scalars_dev must be there and 16-byte aligned");
    if (a.obs && !a.rows) return fail(MATE_EINVAL, "frame_fragment: the %s team's observation rows are missing", kTeamNames[cfg->team]);
    if (a.rows && (a.rows == a.obs || a.rows == a.final_obs)) return fail(MATE_EINVAL, "frame_fragment: the rows and obs_dev / final_obs_dev must be different buffers");
    if ((reinterpret_cast<uintptr_t>(a.rows) & (e->p.obs_f64 ? 7u : 3u)) != 0) return fail(MATE_EINVAL, "frame_fragment: the rows are not aligned to their element");
    a.reward_rows = a.shaped ? (camera ? e->reward.args.cam_rows : e->reward.args.tgt_rows) : nullptr;
    a.phase = phase; a.closes = closes;
    MATE_TRY(enter(e, (hipStream_t)stream, "frame_fragment"));
    note_stream(e, (hipStream_t)stream);
    HIP_TRY(launch_fragment_frame(e->p.obs_f64 != 0, plan_fragment_rows(e).blocks, (hipStream_t)stream, a));
    return MATE_OK;
}
