// render_host.inc -- the host side of the off-screen render (include/mate_engine.h, csrc/render_rows.hpp), included by mate_engine.hip behind frame_host.inc
// (which it shares fail, HIP_TRY, MATE_TRY, enter and note_stream with).  Host only: keeping the mask words, the argument check and the ONE launch.

// The engine's own copy of the mask words without the on-device agents: allocated here once (mate_engine_policy_enable allocates the same buffer), filled
// by every later launch that writes a view.  Ahead of the reset whose pictures matter: until a view is written the words read zero.
extern "C" int mate_engine_keep_masks(mate_engine *e) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (e->g.own_masks) return MATE_OK;
    MATE_TRY(enter_host(e));                   // (no launch in flight reads the record pointers while one of them changes)
    return dev_alloc(e, &e->g.own_masks, (size_t)e->N * e->p.MW);
}

// Identical arguments at every call, no allocation, no synchronisation: every check comes ahead of the first thing that touches the engine.  What is wrong
// with the arguments themselves is reported ahead of what is wrong with the engine's state.
extern "C" int mate_engine_render(mate_engine *e, const int32_t *env_indices_dev, int64_t count, int32_t size, const double *headings_dev, uint8_t *out_dev, void *stream) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    const Params &p = e->p;
    if (count < 1) return fail(MATE_EINVAL, "render: count must be at least 1 (got %lld)", (long long)count);
    if (!env_indices_dev && count > e->N) return fail(MATE_EINVAL, "render: without indices the first `count` environments are drawn: index %lld is outside [0, %lld)", (long long)(count - 1), (long long)e->N);
    if (size < kRenderMinSize || size > kRenderMaxSize) return fail(MATE_EINVAL, "render: size must lie in [%d, %d] (got %d)", kRenderMinSize, kRenderMaxSize, size);
    if (!out_dev || (reinterpret_cast<uintptr_t>(out_dev) & 15u)) return fail(MATE_EINVAL, "render: out_dev must be there and 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(env_indices_dev) & 3u) || (reinterpret_cast<uintptr_t>(headings_dev) & 7u)) return fail(MATE_EINVAL, "render: the indices or the headings are not aligned to their element");
    if (!e->was_reset) return fail(MATE_ESTATE, "render called before reset() (or import_state)");
    if (!e->g.own_masks) return fail(MATE_ESTATE, "render reads the engine's own mask words: mate_engine_keep_masks (or mate_engine_policy_enable) allocates them, ahead of the reset, and every launch that writes a view fills them");
    const int64_t tiles = (int64_t)((size + kRenderTile - 1) / kRenderTile) * ((size + kRenderTile - 1) / kRenderTile);
    if (count > (int64_t)0x7fffffff / tiles) return fail(MATE_EINVAL, "render: %lld frames of %d x %d pixels are more tiles than one launch takes", (long long)count, size, size);
    if (render_slots(p.Nc, p.Nt, p.No) > kRenderMaxSlots) return fail(MATE_EINVAL, "render: the display list of this scenario is longer than %d primitives", kRenderMaxSlots);
    const bool arrows = e->trace.on();         // (the arrows of whichever teams have a communication trace: their part of the LDS only then)
    if (arrows && (p.Nc > 16 || p.Nt > 16)) return fail(MATE_EINVAL, "render: the arrows of a communication trace take teams of at most 16 agents");
    const size_t lds = (size_t)render_lds_bytes(p.Nc, p.Nt, p.No) + (arrows ? (size_t)kRenderArrowBytes : 0);
    if (lds > 64 * 1024) return fail(MATE_EINVAL, "render: the display list does not fit the dynamic LDS a launch has without opting in");
    MATE_TRY(enter(e, (hipStream_t)stream, "render"));
    mate_layout layout;
    MATE_TRY(mate_engine_get_layout(e, &layout));
    RenderArgs a{};
    a.stat = e->g.stat; a.dyn = e->g.dyn; a.knots = e->g.lut_knots; a.bucket = e->g.lut_bucket; a.knot_count = e->g.lut_count;
    a.masks = e->g.own_masks; a.envs = env_indices_dev; a.headings = headings_dev; a.out = out_dev;
    a.N = e->N; a.count = (int32_t)count; a.size = size; a.bit_ct = layout.bit_camera_target; a.bit_tr = layout.bit_target_row;
    for (int team = 0; arrows && team < 2; ++team)
        if (e->trace.team[team].on) { a.trace[team] = e->trace.team[team].d_remaining; a.trace_tags[team] = e->trace.team[team].d_tags; }
    a.duration = e->trace.duration;
    note_stream(e, (hipStream_t)stream);
    HIP_TRY(launch_render(size % kRenderTile == 0, (unsigned)(count * tiles), lds, (hipStream_t)stream, e->d_params, a));
    return MATE_OK;
}
