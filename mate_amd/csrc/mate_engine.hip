// mate_engine.hip -- host side of the C ABI declared in include/mate_engine.h.
// Plain HIP runtime: no torch types cross this boundary (device pointers + sizes only).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <random>
#include <string>
#include <vector>

#include "../../include/mate_engine.h"
#include "reset_kernels.hpp"
#include "policy_kernels.hpp"
#include "aux_kernels.hpp"
#include "engine_host.h"      // (state_rows.hpp, reward_rows.hpp, selection_rows.hpp)

using namespace mate;

static const char *const kTeamNames[2] = {"camera", "target"};      // by MATE_TEAM_*: the error texts' words
static thread_local std::string g_error;
static int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
    return code;
}
// (a failed runtime call leaves HIP's sticky "last error" set: it is read here, so that the next launch check -- ours or the
// caller's, e.g. torch's -- does not report it a second time)
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) { (void)hipGetLastError(); return fail(MATE_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); }    \
    } while (0)
#define MATE_TRY(expr) do { const int rc_ = (expr); if (rc_ != MATE_OK) return rc_; } while (0)      // (an engine function's own status: the error text is set)

// Kernels per (scenario shape, observation type): a compiled specialisation where one exists -- every scenario the reference
// ships, shape_groups.hpp -- else the generic kernels.  step[flow]: the launch-flag specialisations (enum Flow) exist for f32
// observations, the product path; f64 observations (the parity mirror) run the generic flow everywhere.
// `image`: the row-image compilation of the fused random-policy rollout (engine_kernels.hpp: image_statics) where the shape has
// one.  (The fused Greedy rollout keeps the descriptor packer: with the agents' memory next to a 6 KB row image only three
// workgroups fit a CU -- 3072 of the 4096 environments of a MATE-4v8-9 batch resident -- and a second pass costs more than
// the packer's instructions.)
static KernelSet pick_kernels(int Nc, int Nt, int No, bool f64, bool generic, bool no_image) {
    KernelSet k;
    if (!generic && (pick_kernels_group0(Nc, Nt, No, f64, no_image, &k) || pick_kernels_group1(Nc, Nt, No, f64, no_image, &k) ||
                     pick_kernels_group2(Nc, Nt, No, f64, no_image, &k) || pick_kernels_group3(Nc, Nt, No, f64, no_image, &k) ||
                     pick_kernels_group4(Nc, Nt, No, f64, no_image, &k) || pick_kernels_group5(Nc, Nt, No, f64, no_image, &k))) {
        k.specialised = 1;
        return k;
    }
    // the generic set: AnyShape has no row-image form and no sub-wave kernels; its step_greedy_kernel exists
    return f64 ? f64_kernels<AnyShape>() : f32_kernels<AnyShape, void, true>(no_image);
}

static Switches read_switches() {
    Switches w;
    auto flag = [](const char *name) { const char *v = getenv(name); return v && atoi(v) != 0; };
    w.generic = flag("MATE_GENERIC");
    w.flow_generic = flag("MATE_FLOW_GENERIC");
    if (const char *v = getenv("MATE_STAGGER")) w.stagger = atoi(v);
    if (const char *v = getenv("MATE_LUT_SMALL_CAP")) w.lut_small_cap = atoi(v);
    w.reset_monolithic = flag("MATE_RESET_MONOLITHIC");
    if (const char *v = getenv("MATE_ROLLOUT_ROTATE")) w.rollout_rotate = atoi(v);
    w.zoom_iterate = flag("MATE_ZOOM_ITERATE");
    w.policy_split = flag("MATE_POLICY_SPLIT");
    w.step_greedy_rollout = flag("MATE_STEP_GREEDY_ROLLOUT");
    w.no_image = flag("MATE_NO_IMAGE");
    if (const char *v = getenv("MATE_STEP_SUBWAVE")) w.step_sub_wave = atoi(v) != 0;
    if (const char *v = getenv("MATE_SUBWAVE")) w.sub_wave_mode = atoi(v) == 0 ? 0 : 1;
    if (const char *v = getenv("MATE_STEP_SPLIT")) w.step_split = atoi(v) != 0;
    if (const char *v = getenv("MATE_PIPELINED_PRIORITY")) w.pipelined_low_priority = atoi(v) != 0;
    w.pipelined_serial = flag("MATE_PIPELINED_SERIAL");
    if (const char *v = getenv("MATE_HEADLINE_UNIT")) w.headline_unit = atoi(v) != 0;
    return w;
}

// The host-side accessors wait for the stream of the handle's most recent launch, not for the device.  Work the caller enqueued
// through this handle on ANOTHER stream since the last wait, or a stream handle that has been destroyed since, falls back to
// hipDeviceSynchronize: an accessor never reads or writes engine memory under a launch in flight.
static void note_stream(mate_engine *e, hipStream_t stream) {
    if (e->launched && stream != e->last_stream) e->multi_stream = true;
    e->last_stream = stream; e->launched = true;
}
static int leave_pipelined(mate_engine *e, hipStream_t stream);
static hipError_t wait_for_launches(mate_engine *e) {
    if (e->pipelined && leave_pipelined(e, e->last_stream) != MATE_OK) return hipErrorUnknown;      // (resets still running on the side stream)
    hipError_t err = e->multi_stream ? hipErrorInvalidHandle : hipStreamSynchronize(e->last_stream);
    if (err != hipSuccess) { (void)hipGetLastError(); e->last_stream = nullptr; err = hipDeviceSynchronize(); }
    // everything launched so far has drained: the bookkeeping starts afresh (the next launch, on whatever stream, is the only one in flight)
    if (err == hipSuccess) { e->multi_stream = false; e->launched = false; }
    return err;
}

// The opening of an entry point that launches on `stream`: the pipelined-restart mode is left and, for the calls that need an
// episode in progress (`who`: their name in the message), a reset must have run.  Of a host-side accessor: the launches drain.
static int enter(mate_engine *e, hipStream_t stream, const char *who = nullptr) {
    MATE_TRY(leave_pipelined(e, stream));
    if (who && !e->was_reset) return fail(MATE_ESTATE, "%s called before reset() (or import_state)", who);
    HIP_TRY(hipSetDevice(e->device));
    return MATE_OK;
}
static int enter_host(mate_engine *e) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(wait_for_launches(e));
    return MATE_OK;
}

// body(float{}) or body(double{}): the statements that differ by the observation (or row) type only
template <class Body>
static auto with_obs_type(bool f64, Body &&body) { return f64 ? body(double{}) : body(float{}); }

// Opt a kernel in to `bytes` of dynamic LDS (null: a kernel this engine does not have).
static hipError_t set_dynamic_lds(const void *fn, size_t bytes) {
    return fn ? hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) : hipSuccess;
}
template <class... P>
static hipError_t set_dynamic_lds(void (*fn)(P...), size_t bytes) { return set_dynamic_lds(reinterpret_cast<const void *>(fn), bytes); }

// Kernel timing: every e->timing-th eligible launch takes a pair of events from the pool, attached to the dispatch itself
// (the extended launch): the elapsed time is the kernel's own begin->end, without the marker-packet latency separate
// hipEventRecord calls would add.  An untimed launch is a plain one: stream capture records it.
struct Timed { hipEvent_t a = nullptr, b = nullptr; };
static int take_timing_events(mate_engine *e, bool eligible, Timed *out) {
    if (!eligible || e->timing <= 0 || (e->timing_tick++ % e->timing) != 0) return MATE_OK;
    if (e->events_used == e->events.size()) {
        hipEvent_t a, b;
        HIP_TRY(hipEventCreate(&a)); HIP_TRY(hipEventCreate(&b));
        e->events.emplace_back(a, b);
    }
    out->a = e->events[e->events_used].first; out->b = e->events[e->events_used].second; ++e->events_used;
    return MATE_OK;
}
template <class... P>
static void launch(void (*fn)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, Timed t, std::common_type_t<P>... args) {
    if (t.a) hipExtLaunchKernelGGL(fn, grid, block, lds, stream, t.a, t.b, 0, args...);
    else hipLaunchKernelGGL(fn, grid, block, lds, stream, args...);
}

extern "C" const char *mate_engine_last_error(void) { return g_error.c_str(); }
extern "C" int mate_engine_abi_version(void) { return MATE_ABI_VERSION; }

static int next_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }
constexpr int kSortGridCap = 1024;     // workgroups of a table-build launch when the sort arrays live in HBM (one scratch slice each)
static int round_up(int v, int m) { return (v + m - 1) / m * m; }


// LDS carve of the reset kernel behind the wave-0 context: the four sort arrays of the occlusion-table build (keys, values,
// compacted keys, compacted values: 4 x sort_cap doubles), the per-degree index, per-obstacle ray metadata, a scan buffer.
// Up to 20 obstacles per camera table (360 + 185 * obstacles rays) the sort runs in the 160 KiB LDS; beyond, the same code
// sorts in an HBM scratch slice per workgroup (slower: every pass of the bitonic network is a global round trip).
static void layout_reset_lds(const Params &p, ResetLds &rl, int sort_cap) {
    rl.sort_cap = sort_cap;
    const int fixed = 368 * 2 + round_up(8 * p.No * 8 + (2 * p.No + 4) * 4, 16) + 256 * 4;
    rl.sort_in_hbm = (size_t)p.lds_wave_bytes + (size_t)4 * sort_cap * 8 + fixed > kLdsCeiling;
    const int in_lds = rl.sort_in_hbm ? 0 : sort_cap * 8;
    // (the placement phase borrows the start of the sort region for its list of placed circles: keep that much in the LDS)
    const int place_bytes = round_up(5 * (4 + p.Nc + p.No + p.Nt) * 8 + (p.Nc + p.No + 2 * p.Nt) * 4 + 64, 16);
    int roff = p.lds_wave_bytes;
    rl.off_pre = roff + place_bytes;                       // 256 precomputed placement uniforms behind the list of placed circles
    rl.off_keys = roff; roff += std::max(rl.sort_in_hbm ? 0 : in_lds, place_bytes + 2048);
    rl.off_vals = roff; roff += in_lds;
    rl.off_okeys = roff; roff += in_lds;
    rl.off_ovals = roff; roff += in_lds;
    rl.off_bucket = roff; roff += 368 * 2;
    rl.off_meta = roff; roff += round_up(8 * p.No * 8 + (2 * p.No + 4) * 4, 16);
    rl.off_scan = roff; roff += 256 * 4;
    rl.total_bytes = roff;
}

// Two-tier table launches: the worst case (obstacles filling a camera's horizon: 185 rays each) sizes the sort arrays at
// 4 x 2048 doubles = 64 KB, two workgroups per CU, while a table of the shipped scenarios has ~550 rays.  The per-camera
// table launch therefore runs with half-size arrays (four workgroups per CU) and defers the rare larger table to a small
// full-size launch behind it (RESET_PAIRS).  MATE_LUT_SMALL_CAP=<rays> overrides the small size (tests force deferrals with it).
static void setup_two_tier(mate_engine *e) {
    e->rl_small = ResetLds{};
    if (e->rl.sort_in_hbm || e->rl.sort_cap < 1024) return;
    int cap = e->rl.sort_cap / 2;
    if (e->sw.lut_small_cap > 0) cap = std::max(512, round_up(e->sw.lut_small_cap, 64));      // (any multiple of 64 rays: build_lut needs no power of two)
    if (cap >= e->rl.sort_cap) return;
    layout_reset_lds(e->p, e->rl_small, cap);
}

template <typename T>
static int dev_alloc(mate_engine *e, T **out, size_t count, bool zero = true) {
    void *ptr = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    hipError_t err = hipMalloc(&ptr, bytes);
    if (err != hipSuccess) return fail(MATE_ENOMEM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(err));
    if (zero) HIP_TRY(hipMemset(ptr, 0, bytes));
    e->allocs.push_back(ptr);
    *out = reinterpret_cast<T *>(ptr);
    return MATE_OK;
}

// Observation descriptors: for every element of a camera / target row block, which scratch slot
// it copies and which visibility bit gates it (joint_observation, environment.py:908-964).
// Team modes (mate_engine_set_obs_mode): 0 plain; 1 EnhancedObservation = every entity block visible
// (wrappers/enhanced_observation.py:96-125); 2 SharedFieldOfView = opponents and obstacles gated by the team-wide
// flags, teammates always visible (wrappers/shared_field_of_view.py:96-143).
static void build_descriptors(const Params &p, std::vector<uint32_t> &desc, int cam_mode = 0, int tgt_mode = 0) {
    const int Nc = p.Nc, Nt = p.Nt, No = p.No;
    const int sz = p.obs_f64 ? 8 : 4;
    auto D = [&](int src, int flag) { return (uint32_t)(p.off_scratch + src * sz) | ((uint32_t)(p.off_flags + flag * sz) << 16); };   // flag slots: Params::fs_*
    const int ALWAYS = p.fs_always;
    const int SC_ONE = 1, SC_CONST = 2, SC_IDX = 14;      // (slot 0 holds zero)
    desc.assign((size_t)p.tgt_table_off + round_up(p.tgt_elems, 4), D(0, ALWAYS));
    auto preserved = [&](uint32_t *row, int index) {   // environment.py:499-501, 941
        row[0] = D(SC_CONST + 0, ALWAYS); row[1] = D(SC_CONST + 1, ALWAYS); row[2] = D(SC_CONST + 2, ALWAYS);
        row[3] = D(SC_IDX + index, ALWAYS);
        for (int i = 0; i < 9; ++i) row[4 + i] = D(SC_CONST + 3 + i, ALWAYS);
    };
    auto cam_pub = [&](uint32_t *dst, int c, int bit) {   // Camera.state + flag, entities.py:313-321
        for (int i = 0; i < 6; ++i) dst[i] = D(p.sc_cam + c * 10 + i, bit);
        dst[6] = D(SC_ONE, bit);
    };
    auto tgt_pub = [&](uint32_t *dst, int t, int bit) {   // Target.state + flag, entities.py:631-632
        for (int i = 0; i < 4; ++i) dst[i] = D(p.sc_tgt + t * 14 + i, bit);
        dst[4] = D(SC_ONE, bit);
    };
    auto obs_pub = [&](uint32_t *dst, int o, int bit) {   // Obstacle.state + flag
        for (int i = 0; i < 3; ++i) dst[i] = D(p.sc_obs + o * 3 + i, bit);
        dst[3] = D(SC_ONE, bit);
    };
    for (int c = 0; c < Nc; ++c) {
        uint32_t *row = desc.data() + (size_t)c * p.Dc;
        preserved(row, c);
        for (int i = 0; i < 9; ++i) row[13 + i] = D(p.sc_cam + c * 10 + i, ALWAYS);
        uint32_t *q = row + 22;
        for (int t = 0; t < Nt; ++t, q += 5) tgt_pub(q, t, cam_mode == 1 ? ALWAYS : cam_mode == 2 ? p.fs_shared + t : c * Nt + t);
        for (int o = 0; o < No; ++o, q += 4) obs_pub(q, o, cam_mode == 1 ? ALWAYS : cam_mode == 2 ? p.fs_shared + Nt + o : p.fs_camobs + c * No + o);
        for (int c2 = 0; c2 < Nc; ++c2, q += 7) cam_pub(q, c2, cam_mode != 0 ? ALWAYS : p.bit_cc + c * Nc + c2);
    }
    for (int t = 0; t < Nt; ++t) {
        uint32_t *row = desc.data() + p.tgt_table_off + (size_t)t * p.Dt;
        preserved(row, t);
        for (int i = 0; i < 14; ++i) row[13 + i] = D(p.sc_tgt + t * 14 + i, ALWAYS);
        uint32_t *q = row + 27;
        const int rb = p.fs_range + t * p.NJ;
        const int sb = p.fs_shared + Nt + No;
        for (int c = 0; c < Nc; ++c, q += 7) cam_pub(q, c, tgt_mode == 1 ? ALWAYS : tgt_mode == 2 ? sb + c : rb + c);
        for (int o = 0; o < No; ++o, q += 4) obs_pub(q, o, tgt_mode == 1 ? ALWAYS : tgt_mode == 2 ? sb + Nc + o : rb + Nc + o);
        for (int t2 = 0; t2 < Nt; ++t2, q += 5) tgt_pub(q, t2, tgt_mode != 0 ? ALWAYS : rb + Nc + No + t2);
    }
}

template <typename T>
static void build_scratch_init(const Params &p, const mate_config &cfg, std::vector<T> &s) {
    s.assign((size_t)p.nscratch, (T)0);
    s[1] = (T)1;
    s[2] = (T)p.Nc; s[3] = (T)p.Nt; s[4] = (T)p.No;
    const double wh[8] = {925, 925, -925, 925, -925, -925, 925, -925};   // constants.py:70-72
    for (int i = 0; i < 8; ++i) s[5 + i] = (T)wh[i];
    s[13] = (T)75.0;                                                      // constants.py:67
    for (int i = 0; i < 16; ++i) s[14 + i] = (T)i;
    for (int c = 0; c < p.Nc; ++c) {
        T *q = s.data() + p.sc_cam + c * 10;
        q[2] = (T)cfg.camera_radius; q[6] = (T)cfg.camera_max_sight_range;
        q[7] = (T)cfg.camera_rotation_step; q[8] = (T)cfg.camera_zooming_step;
    }
    for (int t = 0; t < p.Nt; ++t) s[p.sc_tgt + t * 14 + 2] = (T)cfg.target_sight_range;
}

extern "C" int mate_engine_create(const mate_config *cfg, int64_t num_envs, int32_t device, uint64_t seed,
                                  uint64_t first_env_index, mate_engine **out) {
    if (!cfg || !out) return fail(MATE_EINVAL, "null argument");
    const int Nc = cfg->num_cameras, Nt = cfg->num_targets, No = cfg->num_obstacles;
    if (Nt < 1) return fail(MATE_EINVAL, "There must be at least one target in the environment.");   // environment.py:220-221
    if (Nc < 0 || Nc > 16 || Nt > 16 || No < 0 || No > 64) return fail(MATE_EINVAL, "unsupported entity counts (%d cameras, %d targets, %d obstacles)", Nc, Nt, No);
    if (num_envs < 1) return fail(MATE_EINVAL, "num_envs must be positive");
    if (cfg->max_episode_steps <= 0) return fail(MATE_EINVAL, "`max_episode_steps` must be a positive integer.");   // environment.py:202-203
    if (cfg->num_cargoes_per_target < 4) return fail(MATE_EINVAL, "`num_cargoes_per_target` should be no less than 4. Got %d.", cfg->num_cargoes_per_target);
    if (!(cfg->high_capacity_target_split >= 0.0 && cfg->high_capacity_target_split <= 1.0)) return fail(MATE_EINVAL, "`high_capacity_target_split` must be between 0 and 1.");
    if (!(cfg->bounty_factor >= 0.0)) return fail(MATE_EINVAL, "`bounty_factor` must be a non-negative number.");
    if (!(cfg->target_step_size > 0.0) || !(cfg->target_sight_range > 0.0)) return fail(MATE_EINVAL, "`target/step_size` and `target/sight_range` must be positive numbers.");
    if (Nc > 0 && (!(cfg->camera_min_viewing_angle > 0.0 && cfg->camera_min_viewing_angle <= 180.0) || !(cfg->camera_rotation_step > 0.0) ||
                   !(cfg->camera_zooming_step > 0.0) || !(cfg->camera_max_sight_range > 0.0) || !(cfg->camera_radius >= 0.0)))
        return fail(MATE_EINVAL, "invalid camera parameters");
    if (!(cfg->transmittance >= 0.0 && cfg->transmittance <= 1.0)) return fail(MATE_EINVAL, "`transmittance` must be within [0, 1]");
    if ((Nc > 0 && !cfg->camera_location_ranges) || !cfg->target_location_ranges || (No > 0 && !cfg->obstacle_location_ranges))
        return fail(MATE_EINVAL, "missing location ranges");
    if (Nc * Nt + Nc * Nc > 0xfff0 || Nt * (Nc + No + Nt) > 0xfff0) return fail(MATE_EINVAL, "mask too large");

    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail(MATE_EHIP, "no HIP device available: the MI355X engine has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(MATE_EINVAL, "device %d out of range (%d visible)", device, ndev);
    HIP_TRY(hipSetDevice(device));

    mate_engine *e = new mate_engine();
    e->cfg = *cfg;
    e->device = device;
    e->N = num_envs;
    Params &p = e->p;
    fill_shape(p, Nc, Nt, No, cfg->obs_dtype == MATE_OBS_F64);
    p.max_episode_steps = cfg->max_episode_steps; p.sparse_reward = cfg->sparse_reward != 0;
    p.num_cargoes_per_target = cfg->num_cargoes_per_target; p.shuffle = cfg->shuffle_entities != 0;
    p.start_with_cargoes = cfg->targets_start_with_cargoes != 0;
    p.n_high = (int)((double)Nt * std::min(std::max(cfg->high_capacity_target_split, 0.0), 1.0));   // environment.py:1530-1533
    p.tau = std::min(std::max(cfg->transmittance, 0.0), 1.0);
    p.cam_radius = cfg->camera_radius; p.theta_min = cfg->camera_min_viewing_angle; p.rmax = cfg->camera_max_sight_range;
    p.rot = cfg->camera_rotation_step; p.zoom = cfg->camera_zooming_step;
    p.area = cfg->camera_min_viewing_angle * (cfg->camera_max_sight_range * cfg->camera_max_sight_range);   // entities.py:285
    p.tgt_step = cfg->target_step_size; p.tgt_sight = cfg->target_sight_range;
    p.freight_scale = std::ceil(2000.0 / cfg->target_step_size);                 // environment.py:521
    p.bounty_scale = std::ceil(p.freight_scale * std::max(0.0, cfg->bounty_factor));   // environment.py:522
    p.reward_scale = p.freight_scale + p.bounty_scale;
    p.max_team_reward = p.reward_scale * cfg->num_cargoes_per_target * Nt;       // environment.py:527-529
    p.obs_r_lo = cfg->obstacle_radius_range[0]; p.obs_r_hi = cfg->obstacle_radius_range[1];
    p.seed_lo = (uint32_t)seed; p.seed_hi = (uint32_t)(seed >> 32); p.first_env = (uint32_t)first_env_index;
    e->step_lds = 4 * (size_t)p.lds_wave_bytes;
    e->sw = read_switches();
    e->k = pick_kernels(Nc, Nt, No, p.obs_f64 != 0, e->sw.generic, e->sw.no_image);
    { Params pi = p; fill_shape(pi, Nc, Nt, No, false, true); e->image_wave_bytes = e->k.image ? (size_t)pi.lds_wave_bytes : (size_t)p.lds_wave_bytes; }
    if (p.lds_wave_bytes > 0xffff) { delete e; return fail(MATE_EINVAL, "scenario too large for 16-bit LDS descriptors"); }
    ResetLds &rl = e->rl;
    layout_reset_lds(p, rl, std::max(512, next_pow2(Nc > 0 ? 360 + No * 185 + 1 : 1)));
    e->reset_lds = (size_t)rl.total_bytes;
    setup_two_tier(e);
    if (e->step_lds > kLdsCeiling || e->reset_lds > kLdsCeiling) {
        const size_t a = e->step_lds, b = e->reset_lds;
        delete e;
        return fail(MATE_EINVAL, "scenario too large for the 160 KiB LDS (%zu / %zu bytes)", a, b);
    }

    int rc = MATE_OK;
    const size_t N = (size_t)num_envs;
    Ptrs &g = e->g;
    g.N = num_envs;
    {   // per-phase wave priorities (phase_prio, engine_kernels.hpp) pay only while the whole batch is resident
        // at once (<= 4 environment-waves per SIMD); beyond that the dispatcher's own staggering of workgroup
        // generations overlaps stores with arithmetic better than any priority scheme (measured: 8192..65536
        // environments run 15-30 % faster without)
        hipDeviceProp_t prop;
        const int64_t cus = hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.multiProcessorCount : 256;
        e->cus = cus;
        // (round 4: with the rows leaving early the priorities cost 3 % at the headline batch on the boxes measured -- off unless asked for)
        const int digits = e->sw.stagger >= 0 ? e->sw.stagger : 0;

        // the two-wave step: where it measured faster -- batches of at most 8 environments per CU (half a generation of the one-wave
        // kernel: 2048 environments on 256 CUs, -3 % random policy, -8 % caller's actions; at 4096 it is 17 % slower, profiles/HISTORY.md 3.1d)
        if (e->sw.step_split < 0) e->sw.step_split = (Nc > 0 && num_envs <= 8 * cus) ? 1 : 0;
        g.stagger = 0;
        if (digits > 0) {
            int d = digits;
            for (int phase = 4; phase >= 0; --phase, d /= 10) g.stagger |= ((d % 10) & 3) << (2 * phase);
            g.stagger |= (int32_t)0x40000000;
        }
        e->split_on = (e->sw.step_split > 0 && Nc > 0) ? 1 : 0;
    }
    do {
        if ((rc = dev_alloc(e, &g.stat, N * p.SW))) break;
        if ((rc = dev_alloc(e, &g.dyn, N * p.DW))) break;
        if ((rc = dev_alloc(e, &g.lut_knots, N * std::max(Nc, 1) * (size_t)p.kmax, false))) break;
        if ((rc = dev_alloc(e, &g.lut_bucket, N * std::max(Nc, 1) * (size_t)p.nbucket))) break;
        if ((rc = dev_alloc(e, &g.lut_count, N * std::max(Nc, 1)))) break;
        if ((rc = dev_alloc(e, &g.lut_deg, N * std::max(Nc, 1) * (size_t)kLutCells * kDegWords, false))) break;
        if ((rc = dev_alloc(e, &g.done_count, (size_t)2))) break;
        if ((rc = dev_alloc(e, &g.done_list, 2 * N))) break;
        if ((rc = dev_alloc(e, &g.flag_count, (size_t)4))) break;
        if ((rc = dev_alloc(e, &g.flag_list, N))) break;
        if ((rc = dev_alloc(e, &g.lut_overflow, N * (size_t)std::max(Nc, 1) + 1))) break;
        if ((rc = dev_alloc(e, &g.idle_steps, N))) break;
        if ((rc = dev_alloc(e, &g.ctrl, (size_t)4))) break;
        if (rl.sort_in_hbm && (rc = dev_alloc(e, &g.sort_scratch, (size_t)kSortGridCap * 4 * rl.sort_cap, false))) break;
        std::vector<uint32_t> desc;
        build_descriptors(p, desc);
        uint32_t *d_desc = nullptr;
        if ((rc = dev_alloc(e, &d_desc, (size_t)p.desc_table_bytes / 4))) break;
        if (hipMemcpy(d_desc, desc.data(), desc.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { rc = fail(MATE_EHIP, "descriptor upload failed"); break; }
        g.desc = d_desc;
        rc = with_obs_type(p.obs_f64 != 0, [&](auto tag) -> int {
            using T = decltype(tag);
            std::vector<T> s; build_scratch_init(p, *cfg, s);
            T *d = nullptr;
            if (const int rc_ = dev_alloc(e, &d, s.size())) return rc_;
            if (hipMemcpy(d, s.data(), s.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return fail(MATE_EHIP, "scratch upload failed");
            g.scratch_init = d;
            return MATE_OK;
        });
        if (rc) break;
        std::vector<double> ranges((size_t)(Nc + No + Nt) * 4, 0.0);
        if (Nc) std::memcpy(ranges.data(), cfg->camera_location_ranges, sizeof(double) * 4 * Nc);
        if (No) std::memcpy(ranges.data() + 4 * Nc, cfg->obstacle_location_ranges, sizeof(double) * 4 * No);
        std::memcpy(ranges.data() + 4 * (Nc + No), cfg->target_location_ranges, sizeof(double) * 4 * Nt);
        double *d_ranges = nullptr;
        if ((rc = dev_alloc(e, &d_ranges, ranges.size()))) break;
        if (hipMemcpy(d_ranges, ranges.data(), ranges.size() * 8, hipMemcpyHostToDevice) != hipSuccess) { rc = fail(MATE_EHIP, "range upload failed"); break; }
        g.reset_ranges = d_ranges;
    } while (0);
    if (rc == MATE_OK) rc = dev_alloc(e, &e->d_params, (size_t)1);
    if (rc == MATE_OK) g.dev_tick_ptr = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(e->d_params) + offsetof(Params, dev_tick));
    if (rc == MATE_OK && hipMemcpy(e->d_params, &e->p, sizeof(Params), hipMemcpyHostToDevice) != hipSuccess) rc = fail(MATE_EHIP, "params upload failed");
    if (rc == MATE_OK) {
        // opt in to large dynamic LDS
        const KernelSet &k = e->k;
        hipError_t err = hipSuccess;
        auto opt_in = [&](auto fn, size_t bytes) { if (err == hipSuccess) err = set_dynamic_lds(fn, bytes); };
        for (int f = 0; f < 3; ++f) opt_in(k.step[f], e->step_lds);
        for (int f = 0; f < 2; ++f) opt_in(k.rollout[f], f == 1 && k.image ? 4 * e->image_wave_bytes : e->step_lds);
        for (int f = 0; f < 3; ++f) opt_in(k.rollout_sub[f], k.sub_wave * e->step_lds);
        if (headline_form(e)) for (int f = 0; f < 2; ++f) opt_in(headline_rollout_function(f), headline_lds_bytes(e->image_wave_bytes));
        with_obs_type(p.obs_f64 != 0, [&](auto tag) { opt_in(&reset_kernel<decltype(tag)>, e->reset_lds); });
        if (err != hipSuccess) rc = fail(MATE_EHIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(err));
    }
    if (rc != MATE_OK) { mate_engine_destroy(e); return rc; }
    *out = e;
    return MATE_OK;
}

extern "C" int mate_engine_destroy(mate_engine *e) {
    if (!e) return MATE_OK;
    (void)hipSetDevice(e->device);
    if (e->side) {                                   // pipelined restarts: nothing of ours may still run when the memory goes
        (void)hipStreamSynchronize(e->side);
        (void)hipStreamDestroy(e->side);
        if (e->ev_launch) (void)hipEventDestroy(e->ev_launch);
        for (int q = 0; q < 2; ++q) if (e->ev_reset[q]) (void)hipEventDestroy(e->ev_reset[q]);
    }
    for (auto &ev : e->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    for (void *ptr : e->allocs) (void)hipFree(ptr);
    delete e;
    return MATE_OK;
}

// (a[i], b[i]) host arrays -> an interleaved (scale, bias) table in the kernels' row type, at `dst` on the device
static int upload_interleaved(void *dst, const double *a, const double *b, size_t n, bool f64) {
    return with_obs_type(f64, [&](auto tag) -> int {
        using T = decltype(tag);
        std::vector<T> ab(2 * n);
        for (size_t i = 0; i < n; ++i) { ab[2 * i] = (T)a[i]; ab[2 * i + 1] = (T)b[i]; }
        HIP_TRY(hipMemcpy(dst, ab.data(), ab.size() * sizeof(T), hipMemcpyHostToDevice));
        return MATE_OK;
    });
}

static int apply_obs_tables(mate_engine *e) {
    const Params &p = e->p;
    std::vector<uint32_t> desc;
    build_descriptors(p, desc, e->team_mode[MATE_TEAM_CAMERA], e->team_mode[MATE_TEAM_TARGET]);
    HIP_TRY(hipMemcpy(const_cast<uint32_t *>(e->g.desc), desc.data(), desc.size() * 4, hipMemcpyHostToDevice));
    e->g.obs_mode = e->team_mode[MATE_TEAM_CAMERA] | (e->team_mode[MATE_TEAM_TARGET] << 2);
    const bool relative = e->xf_relative;
    const double *cam_scale = e->xf_cam ? e->xf_cam_scale.data() : nullptr, *cam_bias = e->xf_cam ? e->xf_cam_bias.data() : nullptr;
    const double *tgt_scale = e->xf_tgt ? e->xf_tgt_scale.data() : nullptr, *tgt_bias = e->xf_tgt ? e->xf_tgt_bias.data() : nullptr;
    if (!relative && !cam_scale && !tgt_scale) { e->g.xdesc = nullptr; e->g.xab = nullptr; return MATE_OK; }
    const size_t n = desc.size();
    const int sz = p.obs_f64 ? 8 : 4;
    const uint32_t zero_slot = (uint32_t)p.off_scratch;   // scratch[0] == 0
    std::vector<uint2> xd(n);
    std::vector<double> a(n, 1.0), b(n, 0.0);
    auto fill = [&](int base, int rows, int D, int self_dim, int own_base, int own_stride, const int (&block)[3], const int (&stride)[3],
                    const double *scale, const double *bias) {
        for (int r = 0; r < rows; ++r) {
            const uint32_t ox = (uint32_t)(p.off_scratch + (own_base + r * own_stride) * sz), oy = ox + (uint32_t)sz;
            for (int col = 0; col < D; ++col) {
                const size_t i = (size_t)base + (size_t)r * D + col;
                uint32_t org = zero_slot;
                if (relative) {
                    if (col >= 4 && col < 12) org = ((col - 4) & 1) ? oy : ox;             // warehouse centres in the preserved block
                    int start = 13 + self_dim;
                    for (int k = 0; k < 3; ++k) {
                        const int width = block[k] * stride[k];
                        if (col >= start && col < start + width) { const int q = (col - start) % stride[k]; if (q == 0) org = ox; else if (q == 1) org = oy; }
                        start += width;
                    }
                }
                xd[i] = make_uint2(desc[i], org);
                if (scale) { a[i] = scale[col]; b[i] = bias[col]; }
            }
        }
    };
    const int cam_blocks[3] = {p.Nt, p.No, p.Nc}, cam_strides[3] = {5, 4, 7};
    const int tgt_blocks[3] = {p.Nc, p.No, p.Nt}, tgt_strides[3] = {7, 4, 5};
    for (size_t i = 0; i < n; ++i) xd[i] = make_uint2(desc[i], zero_slot);
    fill(0, p.Nc, p.Dc, 9, p.sc_cam, 10, cam_blocks, cam_strides, cam_scale, cam_bias);
    fill(p.tgt_table_off, p.Nt, p.Dt, 14, p.sc_tgt, 14, tgt_blocks, tgt_strides, tgt_scale, tgt_bias);
    int rc;
    if (!e->d_xdesc && (rc = dev_alloc(e, &e->d_xdesc, n))) return rc;
    HIP_TRY(hipMemcpy(e->d_xdesc, xd.data(), n * sizeof(uint2), hipMemcpyHostToDevice));
    if (!e->d_xab) {
        unsigned char *buf = nullptr;
        if ((rc = dev_alloc(e, &buf, 2 * n * (size_t)sz))) return rc;
        e->d_xab = buf;
    }
    if ((rc = upload_interleaved(e->d_xab, a.data(), b.data(), n, p.obs_f64 != 0))) return rc;
    e->g.xab = e->d_xab;
    e->g.xdesc = e->d_xdesc;
    return MATE_OK;
}

// Fused observation post-processing tables: descriptor + LDS offset of the row owner's x / y for the
// coordinate entries (coordinate_mask_of, constants.py:371-426) + (scale, bias) per column.
extern "C" int mate_engine_set_obs_transform(mate_engine *e, int32_t relative, const double *cam_scale, const double *cam_bias,
                                             const double *tgt_scale, const double *tgt_bias) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if ((cam_scale && !cam_bias) || (tgt_scale && !tgt_bias)) return fail(MATE_EINVAL, "scale without bias");
    MATE_TRY(enter_host(e));
    const Params &p = e->p;
    e->xf_relative = relative != 0;
    e->xf_cam = cam_scale != nullptr; e->xf_tgt = tgt_scale != nullptr;
    if (cam_scale) { e->xf_cam_scale.assign(cam_scale, cam_scale + p.Dc); e->xf_cam_bias.assign(cam_bias, cam_bias + p.Dc); }
    if (tgt_scale) { e->xf_tgt_scale.assign(tgt_scale, tgt_scale + p.Dt); e->xf_tgt_bias.assign(tgt_bias, tgt_bias + p.Dt); }
    return apply_obs_tables(e);
}

// EnhancedObservation / SharedFieldOfView of the reference (wrappers/enhanced_observation.py,
// wrappers/shared_field_of_view.py) per team, as descriptor variants + a few team-wide flags in the kernel.
extern "C" int mate_engine_set_obs_mode(mate_engine *e, int32_t camera_mode, int32_t target_mode) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (camera_mode < 0 || camera_mode > 2 || target_mode < 0 || target_mode > 2) return fail(MATE_EINVAL, "observation mode must be 0 (plain), 1 (enhanced) or 2 (shared field of view)");
    const int mode[2] = {camera_mode, target_mode};
    for (int team = MATE_TEAM_TARGET; team >= MATE_TEAM_CAMERA; --team)
        if (mode[team] != 0 && e->opponents.kind[team] == MATE_OPPONENT_HEURISTIC)
            return fail(MATE_EINVAL, "set_obs_mode: the heuristic %s opponent (mate_engine_set_%s_opponent) senses the %ss of its plain rows: the %s team mode must stay 0", kTeamNames[team], kTeamNames[team], kTeamNames[1 - team], kTeamNames[team]);
    MATE_TRY(enter_host(e));
    e->team_mode[MATE_TEAM_CAMERA] = camera_mode; e->team_mode[MATE_TEAM_TARGET] = target_mode;
    return apply_obs_tables(e);
}

extern "C" int mate_engine_set_action_grids(mate_engine *e, const double *camera_grid, int32_t n_cam, const double *target_grid, int32_t n_tgt) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (n_cam < 0 || n_tgt < 0 || (n_cam > 0 && !camera_grid) || (n_tgt > 0 && !target_grid)) return fail(MATE_EINVAL, "invalid action grid");
    MATE_TRY(enter_host(e));
    auto upload = [&](const double *src, int n, const double2 **dst, int32_t *count) -> int {
        *dst = nullptr; *count = 0;
        if (n == 0) return MATE_OK;
        double2 *buf = nullptr;
        MATE_TRY(dev_alloc(e, &buf, (size_t)n));
        HIP_TRY(hipMemcpy(buf, src, (size_t)n * sizeof(double2), hipMemcpyHostToDevice));
        *dst = buf; *count = n;
        return MATE_OK;
    };
    int rc = upload(camera_grid, n_cam, &e->g.cam_grid, &e->g.n_cam_grid);
    if (rc == MATE_OK) rc = upload(target_grid, n_tgt, &e->g.tgt_grid, &e->g.n_tgt_grid);
    return rc;
}

extern "C" int mate_engine_get_layout(const mate_engine *e, mate_layout *out) {
    if (!e || !out) return fail(MATE_EINVAL, "null argument");
    const Params &p = e->p;
    out->camera_obs_dim = p.Dc; out->target_obs_dim = p.Dt;
    out->state_dim = 13 + 9 * p.Nc + 14 * p.Nt + 3 * p.No + 2 * p.Nt + 16;   // environment.py:450-466
    out->mask_words = p.MW;
    out->bit_camera_target = 0; out->bit_camera_camera = p.bit_cc; out->bit_target_row = p.bit_range;
    out->bit_camera_obstacle = p.bit_camobs;
    out->export_width = p.export_width; out->lut_capacity = p.kmax; out->scalars_per_env = 8;
    out->specialised = e->k.specialised;
    return MATE_OK;
}

// The episode records' running sums (csrc/episode_rows.hpp) forget the episodes in progress: behind seed() and import_state, whose episode numbers may repeat the tags'.
// Every tag of the table reads NaN: no episode number equals it, the next launch starts every environment's sums from zero
static int clear_episode_sums(mate_engine *e, hipStream_t stream) {
    if (!e->episodes.d_sums) return MATE_OK;
    HIP_TRY(hipMemsetAsync(e->episodes.d_sums, 0xff, (size_t)e->N * kEpisodeWords * sizeof(double), stream));
    return MATE_OK;
}
// The message counts' (tick, episode) tags (csrc/message_rows.hpp) likewise, behind seed(), a reset of the whole batch and import_state: every tag reads
// (-1, -1), the next routing launch zeroes step_edges and total_edges of every environment it runs
static int clear_message_tags(mate_engine *e, hipStream_t stream) {
    for (const Messages::Team &m : e->messages.team)
        if (m.d_tags) HIP_TRY(hipMemsetAsync(m.d_tags, 0xff, sizeof(int32_t) * 2 * (size_t)e->N, stream));
    return MATE_OK;
}

// The communication trace's episode tags (csrc/trace_rows.hpp) likewise, behind seed() and import_state.  Every tag reads -1: no episode number equals it, the next launch starts every environment's matrix from zeros and no arrow is drawn until then.  Behind
// enable, seed() and import_state (whose episode numbers may repeat the tags'); every reset and restart advances the number and needs nothing.
static int clear_trace_tags(mate_engine *e, hipStream_t stream) {
    for (const CommTrace::Team &t : e->trace.team)
        if (t.d_tags) HIP_TRY(hipMemsetAsync(t.d_tags, 0xff, sizeof(int32_t) * (size_t)e->N, stream));
    return MATE_OK;
}

extern "C" int mate_engine_seed(mate_engine *e, uint64_t seed) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (e->dev_tick) return fail(MATE_ESTATE, "seed() while the step counter is device-resident (mate_engine_device_tick)");
    e->p.seed_lo = (uint32_t)seed; e->p.seed_hi = (uint32_t)(seed >> 32);
    MATE_TRY(enter_host(e));
    HIP_TRY(hipMemcpy(e->d_params, &e->p, sizeof(Params), hipMemcpyHostToDevice));
    // the reference re-creates its generators (environment.py:1219-1225): the same seed gives the same episodes again,
    // whatever ran before.  Here: the key, and every counter that enters a Philox counter word (episode, tick) rewound.
    hipLaunchKernelGGL(rewind_kernel, dim3((unsigned)((e->N + 63) / 64)), dim3(64), 0, e->last_stream, (const Params *)e->d_params, (const Ptrs)e->g);
    HIP_TRY(hipGetLastError());
    MATE_TRY(clear_episode_sums(e, e->last_stream));
    MATE_TRY(clear_message_tags(e, e->last_stream));
    MATE_TRY(clear_trace_tags(e, e->last_stream));
    HIP_TRY(wait_for_launches(e));
    e->tick = 0;
    return MATE_OK;
}

static void apply_io(Ptrs &g, const mate_step_io *io) {
    g.cam_act = g.tgt_act = nullptr; g.tape_ct = g.tape_goal = nullptr;
    g.cam_obs = g.tgt_obs = nullptr; g.scalars = nullptr; g.masks = nullptr; g.act_f64 = 0; g.act_discrete = 0;
    if (!io) return;
    g.cam_act = io->camera_actions_dev; g.tgt_act = io->target_actions_dev; g.act_f64 = (io->act_dtype & 0xff) == MATE_ACT_F64 ? 3 : 0;
    g.act_discrete = ((io->act_dtype & MATE_ACT_CAMERA_DISCRETE) ? 1 : 0) | ((io->act_dtype & MATE_ACT_TARGET_DISCRETE) ? 2 : 0);
    g.tape_ct = io->tape_camera_target_dev; g.tape_goal = io->tape_goal_dev;
    g.cam_obs = io->camera_obs_dev; g.tgt_obs = io->target_obs_dev; g.scalars = io->scalars_dev; g.masks = io->masks_dev;
}

// The record pointers of a restart launch: the buffers of `io` receive the restarted environments' first observations and masks
// (null: state only), never `scalars` -- the finished step's reward / done stay -- and nothing is read from a tape.
static Ptrs restart_ptrs(const mate_engine *e, const mate_step_io *io = nullptr) {
    Ptrs r = e->g;
    apply_io(r, io);
    r.scalars = nullptr; r.tape_ct = nullptr; r.tape_goal = nullptr;
    return r;
}

static int launch_reset(mate_engine *e, Ptrs g, int kind, int phases, hipStream_t stream, bool split_done = false) {
    g.mode = MODE_OBSERVE; g.reset_kind = kind; g.parity = e->parity; g.freeze_done = 0;
    note_stream(e, stream);
    const Params &p = e->p;
    auto launch = [&](int ph, int fan, unsigned threads, size_t lds, const ResetLds *layout = nullptr, int64_t grid = 0) {
        int64_t items = ((g.reset_kind == RESET_DONE || g.reset_kind == RESET_LIST) ? std::min<int64_t>(e->N, 256) : e->N) * fan;
        if (e->rl.sort_in_hbm && (ph & PH_LUT)) items = std::min<int64_t>(items, kSortGridCap);     // grid-stride loop; one scratch slice per workgroup
        if (grid > 0) items = grid;
        const ResetLds rl = layout ? *layout : e->rl;
        with_obs_type(p.obs_f64 != 0, [&](auto tag) {
            hipLaunchKernelGGL(reset_kernel<decltype(tag)>, dim3((unsigned)items), dim3(threads), lds, stream, (const Params *)e->d_params, (const Ptrs)g, (const ResetLds)rl, (const int32_t)ph);
        });
    };
    // The immediate auto-reset (RESET_DONE) is launched after EVERY step and is idle almost always: it stays one
    // launch.  Whole-batch, masked and batched (flagged) resets are split -- and so are the list-driven resets of the
    // flows with the on-device greedy agents (`split_done`), whose ~1.2 k-step episodes finish somewhere in the batch all the time:
    // one workgroup per finished environment building its tables one after the other was 9 us per step of the learner-versus-greedy loop
    const uint32_t advance = g.tick_advance;      // device-resident step counter: advanced by the LAST launch of the group
    if ((phases & PH_LUT) && p.Nc > 1 && (kind != RESET_DONE || split_done) && !e->sw.reset_monolithic) {
        g.tick_advance = 0u;
        // placement: one wave per environment; tables: one workgroup per (environment, camera); view: one wave
        // reset_place scratch behind the wave slice: 5 arrays of placed circles + the shuffle permutations
        // (+ the 256 precomputed uniforms of the reset stream behind them)
        const size_t lds_place = (size_t)e->rl.off_pre + 2048;
        if (phases & PH_PLACE) {
            const bool selective = kind == RESET_FLAGGED || kind == RESET_MASK;
            if (selective) HIP_TRY(hipMemsetAsync(g.flag_count, 0, sizeof(int32_t), stream));
            launch(PH_PLACE | PH_MORE, 1, 64, lds_place);
            if (selective) g.reset_kind = RESET_LIST;      // the placement launch listed what it reset
        }
        if (e->rl_small.sort_cap > 0) {
            // tables: small-LDS launch for (almost) all of them, then the full-size launch for what it deferred
            HIP_TRY(hipMemsetAsync(g.lut_overflow, 0, sizeof(int32_t), stream));
            g.lut_defer_above = e->rl_small.sort_cap;
            launch(PH_LUT | PH_PER_CAMERA, p.Nc, 256, (size_t)e->rl_small.total_bytes, &e->rl_small);
            g.lut_defer_above = 0;
            const int kind_now = g.reset_kind;
            g.reset_kind = RESET_PAIRS;
            launch(PH_LUT | PH_PER_CAMERA, 1, 256, e->reset_lds, nullptr, 64);
            g.reset_kind = kind_now;
        } else {
            launch(PH_LUT | PH_PER_CAMERA, p.Nc, 256, e->reset_lds);
        }
        g.tick_advance = advance;
        if (phases & PH_VIEW) launch(PH_VIEW, 1, 64, (size_t)p.lds_wave_bytes);
    } else {
        launch(phases, 1, 256, e->reset_lds);
    }
    HIP_TRY(hipGetLastError());
    return MATE_OK;
}


// ---- attached launches (csrc/state_rows.hpp, reward_rows.hpp, selection_rows.hpp, fragment_rows.hpp)
// Everything a call enqueues around its stepping, reset or import launch while something is attached, in AttachedPlan's order (engine_host.h): the launches it names,
// each with the plan's geometry and capturable (no allocation, no synchronisation, the same arguments at every call); the one check; one function per position.
template <class... P>
static int launch_tiles(void (*fn)(P...), const Tiles &t, hipStream_t stream, std::common_type_t<P>... args) {
    hipLaunchKernelGGL(fn, dim3(t.blocks), dim3(t.threads), t.lds, stream, args...);
    HIP_TRY(hipGetLastError());
    return MATE_OK;
}
static int launch_state_rows(mate_engine *e, const Tiles &t, void *dst, bool f64, const void *ab, hipStream_t stream) {
    return with_obs_type(f64, [&](auto tag) {
        using T = decltype(tag);
        return launch_tiles(state_rows_kernel<T>, t, stream, e->d_params, e->g, reinterpret_cast<T *>(dst), reinterpret_cast<const T *>(ab), t.E);
    });
}
static void launch_soft_coverage(mate_engine *e, const Tiles &t, const uint32_t *masks, double *matrix, double *scores, hipStream_t stream) {
    hipLaunchKernelGGL(soft_coverage_kernel, dim3(t.blocks), dim3(t.threads), t.lds, stream, (const Params *)e->d_params, (const Ptrs)e->g, masks, matrix, scores);
}
static int launch_reward_rows(mate_engine *e, const AttachedPlan &pl, int mode, const float *scalars, const uint32_t *masks, hipStream_t stream) {
    RewardArgs a = e->reward.args;
    a.mode = mode; a.scalars = scalars; a.masks = masks;
    if (mode != REWARD_SNAPSHOT && pl.soft_coverage.blocks)      // (in front where the term exists: every mode but the snapshot)
        launch_soft_coverage(e, pl.soft_coverage, masks, e->reward.d_matrix, e->reward.d_scores, stream);
    return with_obs_type(e->reward.f64, [&](auto tag) { return launch_tiles(reward_rows_kernel<decltype(tag)>, pl.reward_rows, stream, e->d_params, e->g, a); });
}
// (the masks are the engine's own copy, Ptrs::own_masks: every step, reset and restart launch that writes a view writes it there)
static int launch_selection(mate_engine *e, const AttachedPlan &pl, int phase, const float *scalars, hipStream_t stream) {
    SelectionArgs a = e->selection.args;
    a.phase = phase; a.scalars = scalars; a.masks = e->g.own_masks; a.cam_mode = e->team_mode[MATE_TEAM_CAMERA];
    return with_obs_type(e->selection.act_f64, [&](auto tag) { return launch_tiles(selection_kernel<decltype(tag)>, pl.selection, stream, e->d_params, e->g, a); });
}
// `a`: complete arguments (the attached ones with the call's buffers and frames, or the on-demand form's)
static int launch_fragment_rows(mate_engine *e, const Tiles &t, const FragmentArgs &a, bool shaped_f64, hipStream_t stream) {
    return with_obs_type(e->p.obs_f64 != 0, [&](auto obs) {
        return with_obs_type(shaped_f64, [&](auto out) { return launch_tiles(fragment_rows_kernel<decltype(obs), decltype(out)>, t, stream, e->d_params, a); });
    });
}
// 5c: the call's learner steps, its `frames` frames, with the learner's reward row where one describes the step
static int launch_episode_records(mate_engine *e, const AttachedPlan &pl, const mate_step_io *io, int frames, hipStream_t stream) {
    EpisodeArgs a = e->episodes.args;
    const bool camera = a.team == MATE_TEAM_CAMERA;
    a.scalars = io->scalars_dev; a.masks = io->masks_dev; a.K = frames;
    a.dyn = e->g.dyn; a.serial = a.capacity < e->N;
    if (pl.fragment && e->fragment.args.shaped && e->fragment.args.team == a.team) {      // (the fragment's shaped row is the sum over its frames: no row per step)
        a.reward_nan = 1;
    } else if (pl.reward && (camera ? e->reward.args.cam_rows : e->reward.args.tgt_rows)) {      // (the rows of the call's LAST frame, and sums of them in accumulate mode)
        a.rows = camera ? e->reward.args.cam_rows : e->reward.args.tgt_rows; a.rows_f64 = e->reward.f64;
        a.reward_nan = e->reward.accumulate || frames > 1;
    }
    HIP_TRY(launch_episode_rows(pl.episode_rows.blocks, stream, e->d_params, a));
    return MATE_OK;
}
// 3b, 6c: the training-information rows of the step `scalars` / `masks` describe (INFO_STEP; `frames` of the call: more than one and individual_done reads NaN),
// or the snapshot-only form behind new records
static int launch_info(mate_engine *e, const AttachedPlan &pl, int mode, const float *scalars, const uint32_t *masks, int frames, hipStream_t stream) {
    InfoArgs a = e->info.args;
    a.mode = mode; a.scalars = scalars; a.masks = masks; a.done_nan = frames > 1;
    a.dyn = e->g.dyn;
    HIP_TRY(launch_info_rows(pl.info_rows.blocks, pl.info_rows.lds, stream, e->d_params, a));
    return MATE_OK;
}
static int launch_frame_of_call(mate_engine *e, const AttachedPlan &pl, const mate_step_io *io, hipStream_t stream);      // (5', below)
static int launch_trace(mate_engine *e, int freeze_done, hipStream_t stream);      // (2d, trace_host.inc)
// What the attachments ask of a stepping call and what they refuse: made ONCE per call, by the flow the call enters, ahead of everything it enqueues.
// `pipelined`: the call asks for pipelined restarts in a flow that has them; `selected`: it is mate_engine_step_selected (`auto_reset`: its own);
// `fused_team`: it is mate_engine_rollout_versus_greedy for that team (-1: any other call).
static int check_attached_call(const mate_engine *e, const mate_step_io *io, bool pipelined, bool selected, int auto_reset = 0, int fused_team = -1) {
    const char *const no_pipeline = "pipelined restarts (auto_reset = MATE_RESET_PIPELINED) are not available while %s attached (mate_engine_enable_%s): detach %s first";
    if (selected && !e->selection.on) return fail(MATE_ESTATE, "step_selected: call mate_engine_enable_selection() first");
    if (selected && auto_reset < 0) return fail(MATE_ESTATE, "step_selected is not available under pipelined restarts (auto_reset = MATE_RESET_PIPELINED)");
    if (selected && (!io || !io->scalars_dev)) return fail(MATE_EINVAL, "step_selected needs io->scalars_dev (the metrics skip environments whose record says done = 2)");
    if (selected && e->selection.masks_stale) return fail(MATE_ESTATE, "step_selected: the view masks are older than the records (a fused random rollout restarted episodes, or import_state): call observe() first");
    // (the restarts run on the engine's side stream UNDER the next launches: an attached launch on the caller's stream would read records and view masks they rewrite)
    if (pipelined && e->state.on()) return fail(MATE_ESTATE, no_pipeline, "state rows are", "state_rows", "them");
    if (pipelined && e->reward.on) return fail(MATE_ESTATE, no_pipeline, "reward rows are", "reward_rows", "them");
    if (pipelined && e->selection.on) return fail(MATE_ESTATE, no_pipeline, "target selection is", "selection", "it");
    if (e->reward.on && (!io || !io->scalars_dev || !io->masks_dev))      // (the reward launch reads the step's scalar record and masks)
        return fail(MATE_EINVAL, "reward rows are attached (mate_engine_enable_reward_rows): the call needs io->scalars_dev and io->masks_dev");
    if (pipelined && e->fragment.on) return fail(MATE_ESTATE, no_pipeline, "fragment rows are", "fragment_rows", "them");
    if (plan_attached(e, selected, fused_team).fragment) {      // (the fragment launch reads the K scalar records, 16 bytes at a time, the learner's rows and, for a mask term, the masks)
        const void *rows = io ? (fused_team == MATE_TEAM_CAMERA ? io->camera_obs_dev : io->target_obs_dev) : nullptr;
        if (!io || !io->scalars_dev || (reinterpret_cast<uintptr_t>(io->scalars_dev) & 15u) || (e->fragment.args.obs && !rows))
            return fail(MATE_EINVAL, "fragment rows are attached (mate_engine_enable_fragment_rows): the call needs io->scalars_dev, 16-byte aligned, and the learner team's observation rows");
        if (e->fragment.need_masks && !io->masks_dev)
            return fail(MATE_EINVAL, "fragment rows are attached with a mask term (num_tracked / is_tracked): the call needs io->masks_dev");
    }
    if (pipelined && e->frames.on) return fail(MATE_ESTATE, no_pipeline, "per-frame fragments are", "frame_fragments", "them");
    if (pipelined && e->episodes.on) return fail(MATE_ESTATE, no_pipeline, "episode records are", "episode_records", "them");
    if (e->episodes.on) {      // (the episode launch walks the call's scalar records, 16 bytes at a time; the masks are optional: without them num_tracked reads NaN)
        if (!io || !io->scalars_dev || (reinterpret_cast<uintptr_t>(io->scalars_dev) & 15u))
            return fail(MATE_EINVAL, "episode records are attached (mate_engine_enable_episode_records): the call needs io->scalars_dev, 16-byte aligned");
    }
    if (pipelined && e->info.on) return fail(MATE_ESTATE, no_pipeline, "training-information rows are", "info_rows", "them");
    if (pipelined && e->trace.on()) return fail(MATE_ESTATE, no_pipeline, "the communication trace is", "comm_trace", "it");
    if (e->info.on && (!io || !io->scalars_dev || !io->masks_dev))      // (the info launch reads the step's scalar record and masks)
        return fail(MATE_EINVAL, "training-information rows are attached (mate_engine_enable_info_rows): the call needs io->scalars_dev and io->masks_dev");
    return MATE_OK;
}
// 1: ahead of the stepping launch (and of the opponents' agents) -- the executor's joint action of this frame
static int attached_ahead_of_step(mate_engine *e, bool selected, hipStream_t stream) {
    const AttachedPlan pl = plan_attached(e, selected);
    return pl.execute ? launch_selection(e, pl, SELECTION_EXECUTE, nullptr, stream) : MATE_OK;
}
// 3, 3b, 4, 5, 5b, 5c: behind the stepping launch, ahead of the restart of what it finished -- the rows of the launch's last frame (`frames` > 1: rollout-shaped buffers), the fragment of all
// of them, and, with first rows, their scalar records back to "not restarted" (2.0f in every word: only column 2 is read, so no template buffer) -- on EVERY such call, so that no
// environment claims a restart this call did not make
static int attached_behind_step(mate_engine *e, bool selected, const mate_step_io *io, int frames, hipStream_t stream, int fused_team = -1) {
    const AttachedPlan pl = plan_attached(e, selected, fused_team);
    const size_t last = (size_t)(frames - 1) * (size_t)e->N;
    if (pl.reward) {
        MATE_TRY(launch_reward_rows(e, pl, e->reward.accumulate ? REWARD_ACCUMULATE : REWARD_OVERWRITE, io->scalars_dev + last * 8, io->masks_dev + last * e->p.MW, stream));
    }
    if (pl.info) MATE_TRY(launch_info(e, pl, INFO_STEP, io->scalars_dev + last * 8, io->masks_dev + last * e->p.MW, frames, stream));
    if (pl.observe) MATE_TRY(launch_selection(e, pl, SELECTION_OBSERVE, io->scalars_dev + last * 8, stream));
    if (pl.fragment) {
        FragmentArgs a = e->fragment.args;
        a.scalars = io->scalars_dev; a.masks = io->masks_dev; a.K = frames;
        a.rows = a.team == MATE_TEAM_CAMERA ? io->camera_obs_dev : io->target_obs_dev;
        MATE_TRY(launch_fragment_rows(e, pl.fragment_rows, a, e->fragment.f64, stream));
    }
    if (pl.frame) MATE_TRY(launch_frame_of_call(e, pl, io, stream));
    if (pl.first_rows) HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(e->first.scalars), 0x40000000 /* 2.0f */, 8 * (size_t)e->N, stream));
    if (pl.episodes) MATE_TRY(launch_episode_records(e, pl, io, frames, stream));
    return MATE_OK;
}
// 5': the call's frame into the per-frame fragment.  phase: the calls already made inside the open restart interval, modulo K; the call closes the interval
// where its restart follows (restart_finished: auto_reset = 1, or the interval's last call) -- its second form then goes behind that restart (6b')
static int launch_frame_of_call(mate_engine *e, const AttachedPlan &pl, const mate_step_io *io, hipStream_t stream) {
    FrameFragments &f = e->frames;
    FrameArgs a = f.args;
    a.scalars = io->scalars_dev;
    a.rows = f.team == MATE_TEAM_CAMERA ? io->camera_obs_dev : io->target_obs_dev;
    a.reward_rows = a.shaped ? (f.team == MATE_TEAM_CAMERA ? e->reward.args.cam_rows : e->reward.args.tgt_rows) : nullptr;
    a.phase = (int32_t)(e->steps_since_reset % a.K); a.closes = 0;
    f.call_scalars = a.scalars; f.call_rows = a.rows;
    HIP_TRY(launch_fragment_frame(e->p.obs_f64 != 0, pl.frame_rows.blocks, stream, a));
    return MATE_OK;
}
static int launch_frame_first_rows(mate_engine *e, const AttachedPlan &pl, hipStream_t stream) {
    FrameArgs a = e->frames.args;
    a.scalars = e->frames.call_scalars; a.rows = e->frames.call_rows; a.reward_rows = nullptr;
    a.phase = a.K - 1; a.closes = 1;
    HIP_TRY(launch_fragment_frame(e->p.obs_f64 != 0, pl.frame_rows.blocks, stream, a));
    return MATE_OK;
}
// One K = 1 launch of the fragment kernel over the first-row records: the rows of `src` through `columns` into `dst`, for exactly the environments whose record the restart
// launch has just written (column 2 = 0; everywhere else the memset's 2.0f: "no live frame", row not written).  No other output.
static int launch_first_rows(mate_engine *e, const Tiles &t, const void *src, void *dst, const void *columns, hipStream_t stream) {
    FragmentArgs a = e->fragment.args;
    a.scalars = e->first.scalars; a.masks = nullptr; a.rows = src; a.obs = dst; a.columns = columns; a.K = 1;
    a.rewards = a.info = nullptr; a.done = nullptr; a.frames = nullptr; a.shaped = nullptr;
    return launch_fragment_rows(e, t, a, e->fragment.f64, stream);
}
// 6b, 6c: behind a restart launch, a reset or an import.  6b (`fused_team`: the restart is the one mate_engine_rollout_versus_greedy for that team has just enqueued, -1: any
// other) -- the restarted environments' fragment row moves to final_obs where asked for, then their first row goes through the fragment's transform into its place.
// 6c -- the goals and episodes the next step's sparse_delivery (reward rows) and individual_done (info rows) are measured against
static int attached_behind_restart(mate_engine *e, hipStream_t stream, int fused_team = -1) {
    const AttachedPlan pl = plan_attached(e, false, fused_team);
    if (pl.first_rows) {
        void *const obs = e->fragment.args.obs;
        if (e->first.final_obs) MATE_TRY(launch_first_rows(e, pl.fragment_rows, obs, e->first.final_obs, nullptr, stream));
        MATE_TRY(launch_first_rows(e, pl.fragment_rows, e->first.rows, obs, e->fragment.args.columns, stream));
    }
    if (pl.frame_first) MATE_TRY(launch_frame_first_rows(e, pl, stream));
    if (pl.reward) MATE_TRY(launch_reward_rows(e, pl, REWARD_SNAPSHOT, nullptr, nullptr, stream));
    return pl.info ? launch_info(e, pl, INFO_SNAPSHOT, nullptr, nullptr, 1, stream) : MATE_OK;
}
// 7, 8: the LAST launches of every call that leaves new records (`rc`: what it returned so far), behind its auto-reset launch: a restarted environment's rows show the new episode
static int attached_last(mate_engine *e, int rc, hipStream_t stream) {
    if (rc != MATE_OK) return rc;
    const AttachedPlan pl = plan_attached(e, false);
    if (pl.action_mask) MATE_TRY(launch_selection(e, pl, SELECTION_ACTION_MASK, nullptr, stream));
    return pl.state ? launch_state_rows(e, pl.state_rows, e->state.dst, e->state.f64, e->state.ab, stream) : MATE_OK;
}
// 6 .. 8 behind reset, reset_tape and import_state: new records without a step
static int attached_behind_new_records(mate_engine *e, hipStream_t stream) { return attached_last(e, attached_behind_restart(e, stream), stream); }

// ---- global state rows: attaching, and the on-demand launch
// (scale, bias) host arrays -> the kernel's interleaved table in the row type
static int upload_state_table(mate_engine *e, void **table, const double *scale, const double *bias, bool f64) {
    const int S = state_dim_of(e->p.Nc, e->p.Nt, e->p.No);
    if (!*table) {
        unsigned char *buf = nullptr;
        MATE_TRY(dev_alloc(e, &buf, (size_t)2 * S * 8));
        *table = buf;
    }
    return upload_interleaved(*table, scale, bias, (size_t)S, f64);
}

static int check_state_rows_args(const mate_engine *e, const void *dst, int32_t out_dtype, const double *scale, const double *bias) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (out_dtype != MATE_OBS_F32 && out_dtype != MATE_OBS_F64) return fail(MATE_EINVAL, "state rows: out_dtype must be MATE_OBS_F32 or MATE_OBS_F64");
    if ((scale != nullptr) != (bias != nullptr)) return fail(MATE_EINVAL, "state rows: scale without bias (or bias without scale)");
    if (reinterpret_cast<uintptr_t>(dst) & 15u) return fail(MATE_EINVAL, "state rows: the output buffer must be 16-byte aligned");
    return MATE_OK;
}

extern "C" int mate_engine_enable_state_rows(mate_engine *e, void *dst_dev, int32_t out_dtype, const double *scale, const double *bias) {
    MATE_TRY(check_state_rows_args(e, dst_dev, out_dtype, scale, bias));
    if (!dst_dev) { e->state.dst = nullptr; e->state.ab = nullptr; return MATE_OK; }
    if (!e->was_reset) return fail(MATE_ESTATE, "enable_state_rows called before reset() (or import_state)");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(wait_for_launches(e));      // (leaves the pipelined-restart mode; no launch reads the table while it is rewritten)
    const bool f64 = out_dtype == MATE_OBS_F64;
    if (scale) MATE_TRY(upload_state_table(e, &e->state.d_ab, scale, bias, f64));
    e->state.dst = dst_dev; e->state.f64 = f64; e->state.ab = scale ? e->state.d_ab : nullptr;
    return MATE_OK;
}

extern "C" int mate_engine_state_rows(mate_engine *e, void *dst_dev, int32_t out_dtype, const double *scale, const double *bias, void *stream) {
    MATE_TRY(check_state_rows_args(e, dst_dev, out_dtype, scale, bias));
    if (!dst_dev) return fail(MATE_EINVAL, "state_rows: null output buffer");
    MATE_TRY(enter(e, (hipStream_t)stream, "state_rows"));
    const bool f64 = out_dtype == MATE_OBS_F64;
    if (scale) {      // the table of the previous call is kept: the same map again costs no upload and no wait
        const int S = state_dim_of(e->p.Nc, e->p.Nt, e->p.No);
        std::vector<double> table((size_t)2 * S + 1);
        std::copy(scale, scale + S, table.begin()); std::copy(bias, bias + S, table.begin() + S); table[(size_t)2 * S] = f64 ? 1.0 : 0.0;
        if (table.size() != e->state.demand_table.size() || std::memcmp(table.data(), e->state.demand_table.data(), table.size() * 8) != 0) {
            HIP_TRY(wait_for_launches(e));      // (an earlier on-demand launch may still read the old table)
            e->state.demand_table.clear();
            MATE_TRY(upload_state_table(e, &e->state.d_ab_demand, scale, bias, f64));
            e->state.demand_table = table;
        }
    }
    note_stream(e, (hipStream_t)stream);
    return launch_state_rows(e, plan_state_rows(e, f64), dst_dev, f64, scale ? e->state.d_ab_demand : nullptr, (hipStream_t)stream);
}

// ---- shaped reward rows: attaching
extern "C" int mate_engine_enable_reward_rows(mate_engine *e, const mate_reward_rows *cfg) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (!cfg) { e->reward.on = false; return MATE_OK; }
    if (!e->was_reset) return fail(MATE_ESTATE, "enable_reward_rows called before reset() (or import_state)");
    const Params &p = e->p;
    const bool f64 = cfg->out_dtype == MATE_OBS_F64;
    if (cfg->out_dtype != MATE_OBS_F32 && !f64) return fail(MATE_EINVAL, "reward rows: out_dtype must be MATE_OBS_F32 or MATE_OBS_F64");
    if (!cfg->camera_rows_dev && !cfg->target_rows_dev) return fail(MATE_EINVAL, "reward rows: no team (both row buffers are null)");
    if (cfg->camera_rows_dev && p.Nc == 0) return fail(MATE_EINVAL, "reward rows: the scenario has no cameras to shape rewards for");
    if ((cfg->camera_rows_dev && !cfg->camera_coefficients_dev) || (cfg->target_rows_dev && !cfg->target_coefficients_dev))
        return fail(MATE_EINVAL, "reward rows: a team without its coefficient table");
    if ((cfg->camera_terms_dev && !cfg->camera_rows_dev) || (cfg->target_terms_dev && !cfg->target_rows_dev))
        return fail(MATE_EINVAL, "reward rows: term rows without that team's reward rows");
    const uintptr_t row_align = f64 ? 7u : 3u;
    auto misaligned = [](const void *ptr, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(ptr) & mask) != 0; };
    if (misaligned(cfg->camera_rows_dev, row_align) || misaligned(cfg->target_rows_dev, row_align) || misaligned(cfg->camera_terms_dev, 7u) ||
        misaligned(cfg->target_terms_dev, 7u) || misaligned(cfg->camera_coefficients_dev, 7u) || misaligned(cfg->target_coefficients_dev, 7u))
        return fail(MATE_EINVAL, "reward rows: a buffer is not aligned to its element size");
    if (cfg->camera_reduction < MATE_REDUCE_NONE || cfg->camera_reduction > MATE_REDUCE_MIN)
        return fail(MATE_EINVAL, "reward rows: camera_reduction must be one of MATE_REDUCE_NONE .. MATE_REDUCE_MIN");
    if (cfg->target_reduction < MATE_REDUCE_NONE || cfg->target_reduction > MATE_REDUCE_MAX)
        return fail(MATE_EINVAL, "reward rows: target_reduction must be one of MATE_REDUCE_NONE .. MATE_REDUCE_MAX");
    if (cfg->soft_coverage && p.Nc == 0) return fail(MATE_EINVAL, "reward rows: soft_coverage_score needs cameras");
    if (cfg->soft_coverage && !e->g.lut_knots_outer) return fail(MATE_ESTATE, "reward rows: soft_coverage_score needs the outer boundary (mate_engine_enable_outer_boundary)");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(wait_for_launches(e));      // (leaves the pipelined-restart mode; no launch reads the arguments while they change)
    int rc = MATE_OK;
    RewardRows &r = e->reward;
    if (!r.d_snapshot && (rc = dev_alloc(e, &r.d_snapshot, (size_t)e->N * (p.Nt + 1)))) return rc;
    if (cfg->soft_coverage && !r.d_matrix) {
        if ((rc = dev_alloc(e, &r.d_matrix, (size_t)e->N * p.Nc * p.Nt))) return rc;
        if ((rc = dev_alloc(e, &r.d_scores, (size_t)e->N * p.Nc))) return rc;
    }
    mate_layout layout;
    if ((rc = mate_engine_get_layout(e, &layout))) return rc;
    RewardArgs a{};
    a.snapshot = r.d_snapshot;
    a.cam_rows = cfg->camera_rows_dev; a.tgt_rows = cfg->target_rows_dev;
    a.cam_terms = cfg->camera_terms_dev; a.tgt_terms = cfg->target_terms_dev;
    a.cam_coef = cfg->camera_coefficients_dev; a.tgt_coef = cfg->target_coefficients_dev;
    a.soft_matrix = cfg->soft_coverage ? r.d_matrix : nullptr; a.soft_scores = cfg->soft_coverage ? r.d_scores : nullptr;
    a.cam_reduction = cfg->camera_reduction; a.tgt_reduction = cfg->target_reduction;
    a.bit_ct = layout.bit_camera_target;
    r.args = a; r.f64 = f64; r.soft = cfg->soft_coverage != 0; r.accumulate = cfg->accumulate != 0;
    r.on = true;
    // the goals and episodes of the records as they are: the first step's sparse_delivery is measured against them
    note_stream(e, e->last_stream);
    return attached_behind_restart(e, e->last_stream);
}

// ---- FrameSkip fragments: attaching, the coefficient table, and the on-demand launch
// Validates `cfg`, uploads its tables into the given engine-owned buffers (allocated on first use) and fills the launch's arguments but the call's own.
static int fragment_args_of(mate_engine *e, const mate_fragment_rows *cfg, double **d_coef, void **d_columns, FragmentArgs *out, bool *shaped_f64, bool *need_masks) {
    const Params &p = e->p;
    static const char *const kCameraKeys[kRewardCameraTerms] = {"raw_reward", "coverage_rate", "real_coverage_rate", "mean_transport_rate", "soft_coverage_score", "num_tracked", "baseline"};
    static const char *const kTargetKeys[kRewardTargetTerms] = {"raw_reward", "coverage_rate", "real_coverage_rate", "mean_transport_rate", "normalized_goal_distance",
                                                                "sparse_delivery", "soft_coverage_score", "is_tracked", "is_colliding", "baseline"};
    if (cfg->team != MATE_TEAM_CAMERA && cfg->team != MATE_TEAM_TARGET) return fail(MATE_EINVAL, "fragment rows: team must be MATE_TEAM_CAMERA or MATE_TEAM_TARGET");
    const bool camera = cfg->team == MATE_TEAM_CAMERA;
    if (camera && p.Nc == 0) return fail(MATE_EINVAL, "fragment rows: the scenario has no cameras to learn for");
    const bool f64 = cfg->out_dtype == MATE_OBS_F64;
    if (cfg->out_dtype != MATE_OBS_F32 && !f64) return fail(MATE_EINVAL, "fragment rows: out_dtype must be MATE_OBS_F32 or MATE_OBS_F64");
    if (cfg->reduction < MATE_REDUCE_NONE || cfg->reduction > (camera ? MATE_REDUCE_MIN : MATE_REDUCE_MAX))
        return fail(MATE_EINVAL, "fragment rows: reduction must be one of MATE_REDUCE_NONE .. %s", camera ? "MATE_REDUCE_MIN" : "MATE_REDUCE_MAX");
    if (cfg->shaped_dev && !cfg->coefficients) return fail(MATE_EINVAL, "fragment rows: shaped rows without the coefficient table");
    const int have = (cfg->column_sub != nullptr) + (cfg->column_flag != nullptr) + (cfg->column_scale != nullptr) + (cfg->column_bias != nullptr);
    if (have != 0 && have != 4) return fail(MATE_EINVAL, "fragment rows: a partial column table (column_sub, column_flag, column_scale and column_bias go together)");
    const int terms = camera ? kRewardCameraTerms : kRewardTargetTerms, D = camera ? p.Dc : p.Dt;
    const char *const *keys = camera ? kCameraKeys : kTargetKeys;
    bool masks = false;
    for (int k = 0; cfg->coefficients && k < terms; ++k) {
        const bool state_term = camera ? k == 4 : (k == 4 || k == 5 || k == 6 || k == 8);
        if (state_term && cfg->coefficients[k] != 0.0)
            return fail(MATE_EINVAL, "fragment rows: the term %s needs the state of every frame and is not available in a fragment (its coefficient must be 0)", keys[k]);
        if (k == (camera ? 5 : 7) && cfg->coefficients[k] != 0.0) masks = true;
    }
    const uintptr_t obs_align = p.obs_f64 ? 7u : 3u, row_align = f64 ? 7u : 3u;
    auto misaligned = [](const void *ptr, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(ptr) & mask) != 0; };
    if (misaligned(cfg->obs_dev, obs_align) || misaligned(cfg->rewards_dev, 7u) || misaligned(cfg->info_dev, 7u) || misaligned(cfg->frames_dev, 3u) || misaligned(cfg->shaped_dev, row_align))
        return fail(MATE_EINVAL, "fragment rows: a buffer is not aligned to its element size");
    for (int k = 0; have && k < D; ++k)
        if (cfg->column_sub[k] < 0 || cfg->column_sub[k] > 2 || cfg->column_flag[k] < -1 || cfg->column_flag[k] >= D)
            return fail(MATE_EINVAL, "fragment rows: column %d of the table is out of range (sub 0 .. 2, flag -1 .. D - 1)", k);
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(wait_for_launches(e));      // (leaves the pipelined-restart mode; no launch reads the tables while they are rewritten)
    int rc = MATE_OK;
    if (!*d_coef && (rc = dev_alloc(e, d_coef, (size_t)kRewardTargetTerms))) return rc;
    if (!*d_columns) {
        unsigned char *buf = nullptr;
        if ((rc = dev_alloc(e, &buf, (size_t)(p.Dc > p.Dt ? p.Dc : p.Dt) * sizeof(FragmentColumn<double>)))) return rc;
        *d_columns = buf;
    }
    if (cfg->coefficients) HIP_TRY(hipMemcpy(*d_coef, cfg->coefficients, sizeof(double) * terms, hipMemcpyHostToDevice));
    if (have) {
        rc = with_obs_type(p.obs_f64 != 0, [&](auto tag) -> int {
            using T = decltype(tag);
            std::vector<FragmentColumn<T>> table((size_t)D);
            for (int k = 0; k < D; ++k) table[k] = {cfg->column_sub[k], cfg->column_flag[k], (T)cfg->column_scale[k], (T)cfg->column_bias[k]};
            HIP_TRY(hipMemcpy(*d_columns, table.data(), table.size() * sizeof(table[0]), hipMemcpyHostToDevice));
            return MATE_OK;
        });
        if (rc != MATE_OK) return rc;
    }
    mate_layout layout;
    if ((rc = mate_engine_get_layout(e, &layout))) return rc;
    FragmentArgs a{};
    a.obs = cfg->obs_dev; a.columns = have ? *d_columns : nullptr;
    a.rewards = cfg->rewards_dev; a.info = cfg->info_dev; a.done = cfg->done_dev; a.frames = cfg->frames_dev;
    a.shaped = cfg->shaped_dev; a.coef = *d_coef;
    a.N = e->N; a.K = 1; a.team = cfg->team; a.A = camera ? p.Nc : p.Nt; a.D = D; a.reduction = cfg->reduction;
    a.bit_ct = layout.bit_camera_target;
    *out = a; *shaped_f64 = f64; *need_masks = masks && cfg->shaped_dev;
    return MATE_OK;
}

extern "C" int mate_engine_enable_fragment_rows(mate_engine *e, const mate_fragment_rows *cfg) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (!cfg) { e->fragment.on = false; e->first = FirstRows{}; return MATE_OK; }
    if (!e->was_reset) return fail(MATE_ESTATE, "enable_fragment_rows called before reset() (or import_state)");
    FragmentRows &f = e->fragment;
    FragmentArgs a{};
    bool f64 = false, masks = false;
    MATE_TRY(fragment_args_of(e, cfg, &f.d_coef, &f.d_columns, &a, &f64, &masks));
    if (!f.on || a.team != f.args.team || !a.obs) e->first = FirstRows{};      // (first rows complete the rows of ONE team's fragment: another team, or no rows, detaches them)
    f.args = a; f.f64 = f64; f.need_masks = masks;
    f.on = true;
    return MATE_OK;
}

// First rows of restarted episodes: see include/mate_engine.h.  Host state only -- the launches read it when they are enqueued.
extern "C" int mate_engine_enable_first_rows(mate_engine *e, const mate_first_rows *cfg) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (!cfg) { e->first = FirstRows{}; return MATE_OK; }
    if (!e->fragment.on || !e->fragment.args.obs)
        return fail(MATE_ESTATE, "enable_first_rows: fragment rows with obs_dev must be attached first (mate_engine_enable_fragment_rows)");
    auto misaligned = [](const void *ptr, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(ptr) & mask) != 0; };
    if (!cfg->rows_dev || !cfg->scalars_dev || misaligned(cfg->rows_dev, 15u) || misaligned(cfg->scalars_dev, 15u))
        return fail(MATE_EINVAL, "first rows: rows_dev and scalars_dev must be there and 16-byte aligned");
    if (misaligned(cfg->final_obs_dev, e->p.obs_f64 ? 7u : 3u)) return fail(MATE_EINVAL, "first rows: final_obs_dev is not aligned to its element size");
    if (cfg->rows_dev == e->fragment.args.obs || cfg->final_obs_dev == e->fragment.args.obs || cfg->final_obs_dev == cfg->rows_dev)
        return fail(MATE_EINVAL, "first rows: rows_dev, final_obs_dev and the fragment's obs_dev must be three buffers");
    e->first.rows = cfg->rows_dev; e->first.scalars = cfg->scalars_dev; e->first.final_obs = cfg->final_obs_dev;
    e->first.on = true;
    return MATE_OK;
}

// ---- per-episode metric records: attaching, and forgetting the episodes in progress (include/mate_engine.h, csrc/episode_rows.hpp)
extern "C" int mate_engine_enable_episode_records(mate_engine *e, int32_t team, double *records_dev, int64_t capacity, int64_t *count_dev) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (!records_dev) { e->episodes.on = false; return MATE_OK; }
    if (!e->was_reset) return fail(MATE_ESTATE, "enable_episode_records called before reset() (or import_state)");
    if (team != MATE_TEAM_CAMERA && team != MATE_TEAM_TARGET) return fail(MATE_EINVAL, "episode records: team must be MATE_TEAM_CAMERA or MATE_TEAM_TARGET");
    if (team == MATE_TEAM_CAMERA && e->p.Nc == 0) return fail(MATE_EINVAL, "episode records: the scenario has no cameras to keep records for");
    if (capacity < 1) return fail(MATE_EINVAL, "episode records: capacity must be at least 1");
    if (!count_dev) return fail(MATE_EINVAL, "episode records: null counter");
    if ((reinterpret_cast<uintptr_t>(records_dev) | reinterpret_cast<uintptr_t>(count_dev)) & 7u) return fail(MATE_EINVAL, "episode records: the ring and the counter must be 8-byte aligned");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(wait_for_launches(e));      // (leaves the pipelined-restart mode; no launch reads the arguments while they change)
    EpisodeRecords &r = e->episodes;
    { int rc = MATE_OK; if (!r.d_sums && (rc = dev_alloc(e, &r.d_sums, (size_t)e->N * kEpisodeWords, false))) return rc; }
    mate_layout layout;
    MATE_TRY(mate_engine_get_layout(e, &layout));
    EpisodeArgs a{};
    a.sums = r.d_sums; a.records = records_dev; a.count = reinterpret_cast<unsigned long long *>(count_dev);
    a.capacity = capacity; a.N = e->N; a.team = team; a.A = team == MATE_TEAM_CAMERA ? e->p.Nc : e->p.Nt;
    a.bit_ct = layout.bit_camera_target;
    r.args = a;
    r.on = true;
    note_stream(e, e->last_stream);
    return clear_episode_sums(e, e->last_stream);
}
extern "C" int mate_engine_clear_episode_records(mate_engine *e, void *stream) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    MATE_TRY(enter(e, (hipStream_t)stream, "clear_episode_records"));
    note_stream(e, (hipStream_t)stream);
    return clear_episode_sums(e, (hipStream_t)stream);
}

// ---- MoreTrainingInformation rows: attaching, and the on-demand launch (include/mate_engine.h, csrc/info_rows.hpp)
static int check_info_buffers(const mate_engine *e, const double *camera_rows, const double *target_rows, const double *cargo_rows) {
    if ((reinterpret_cast<uintptr_t>(camera_rows) | reinterpret_cast<uintptr_t>(target_rows) | reinterpret_cast<uintptr_t>(cargo_rows)) & 15u)
        return fail(MATE_EINVAL, "info rows: the row buffers must be 16-byte aligned");
    if (camera_rows && e->p.Nc == 0) return fail(MATE_EINVAL, "info rows: the scenario has no cameras to write camera rows for");
    return MATE_OK;
}
extern "C" int mate_engine_enable_info_rows(mate_engine *e, double *camera_rows_dev, double *target_rows_dev, double *cargo_rows_dev) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (!camera_rows_dev && !target_rows_dev && !cargo_rows_dev) { e->info.on = false; return MATE_OK; }
    if (!e->was_reset) return fail(MATE_ESTATE, "enable_info_rows called before reset() (or import_state)");
    MATE_TRY(check_info_buffers(e, camera_rows_dev, target_rows_dev, cargo_rows_dev));
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(wait_for_launches(e));      // (leaves the pipelined-restart mode; no launch reads the arguments while they change)
    InfoRows &r = e->info;
    { int rc = MATE_OK; if (!r.d_snapshot && (rc = dev_alloc(e, &r.d_snapshot, (size_t)e->N * (e->p.Nt + 1)))) return rc; }
    mate_layout layout;
    MATE_TRY(mate_engine_get_layout(e, &layout));
    InfoArgs a{};
    a.snapshot = r.d_snapshot; a.cam_rows = camera_rows_dev; a.tgt_rows = target_rows_dev; a.cargo_rows = cargo_rows_dev;
    a.N = e->N; a.bit_ct = layout.bit_camera_target; a.bit_tr = layout.bit_target_row;
    r.args = a;
    r.on = true;
    // the goals and episodes of the records as they are: the first step's individual_done is measured against them
    note_stream(e, e->last_stream);
    return launch_info(e, plan_attached(e, false), INFO_SNAPSHOT, nullptr, nullptr, 1, e->last_stream);
}
extern "C" int mate_engine_info_rows(mate_engine *e, const uint32_t *masks_dev, double *camera_rows_dev, double *target_rows_dev, double *cargo_rows_dev, void *stream) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (!camera_rows_dev && !target_rows_dev && !cargo_rows_dev) return fail(MATE_EINVAL, "info_rows: no output buffer");
    MATE_TRY(check_info_buffers(e, camera_rows_dev, target_rows_dev, cargo_rows_dev));
    MATE_TRY(enter(e, (hipStream_t)stream, "info_rows"));
    mate_layout layout;
    MATE_TRY(mate_engine_get_layout(e, &layout));
    InfoArgs a{};
    a.mode = INFO_ON_DEMAND; a.masks = masks_dev; a.dyn = e->g.dyn;
    a.cam_rows = camera_rows_dev; a.tgt_rows = target_rows_dev; a.cargo_rows = cargo_rows_dev;
    a.N = e->N; a.bit_ct = layout.bit_camera_target; a.bit_tr = layout.bit_target_row;
    note_stream(e, (hipStream_t)stream);
    const Tiles t = plan_info_rows(e);
    HIP_TRY(launch_info_rows(t.blocks, t.lds, (hipStream_t)stream, e->d_params, a));
    return MATE_OK;
}

extern "C" int mate_engine_fragment_coefficients(mate_engine *e, double **coefficients_dev, int32_t *count) {
    if (!e || !coefficients_dev) return fail(MATE_EINVAL, "null argument");
    if (!e->fragment.on) return fail(MATE_ESTATE, "fragment_coefficients: mate_engine_enable_fragment_rows has not run");
    *coefficients_dev = e->fragment.d_coef;
    if (count) *count = e->fragment.args.team == MATE_TEAM_CAMERA ? kRewardCameraTerms : kRewardTargetTerms;
    return MATE_OK;
}

extern "C" int mate_engine_fragment_rows(mate_engine *e, const mate_fragment_rows *cfg, const mate_step_io *rows, int32_t frames, void *stream) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (!cfg || !rows) return fail(MATE_EINVAL, "fragment_rows: null config or buffers");
    if (frames < 1) return fail(MATE_EINVAL, "fragment_rows: frames must be at least 1");
    MATE_TRY(enter(e, (hipStream_t)stream, "fragment_rows"));
    FragmentRows &f = e->fragment;
    FragmentArgs a{};
    bool f64 = false, masks = false;
    MATE_TRY(fragment_args_of(e, cfg, &f.d_coef_demand, &f.d_columns_demand, &a, &f64, &masks));
    a.rows = cfg->team == MATE_TEAM_CAMERA ? rows->camera_obs_dev : rows->target_obs_dev;
    a.scalars = rows->scalars_dev; a.masks = rows->masks_dev; a.K = frames;
    if (!a.scalars || (reinterpret_cast<uintptr_t>(a.scalars) & 15u)) return fail(MATE_EINVAL, "fragment_rows: scalars_dev must be there and 16-byte aligned");
    if (a.obs && !a.rows) return fail(MATE_EINVAL, "fragment_rows: the learner team's observation rows are missing");
    if (masks && !a.masks) return fail(MATE_EINVAL, "fragment_rows: a mask term (num_tracked / is_tracked) needs masks_dev");
    note_stream(e, (hipStream_t)stream);
    return launch_fragment_rows(e, plan_fragment_rows(e), a, f64, (hipStream_t)stream);
}

extern "C" int mate_engine_reset(mate_engine *e, const uint8_t *env_mask_dev, const mate_step_io *io, void *stream) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    MATE_TRY(enter(e, (hipStream_t)stream));
    Ptrs g = e->g;
    apply_io(g, io);
    g.tape_ct = nullptr; g.tape_goal = nullptr;
    g.reset_mask = env_mask_dev;
    MATE_TRY(launch_reset(e, g, env_mask_dev ? RESET_MASK : RESET_ALL, PH_PLACE | PH_LUT | PH_VIEW, (hipStream_t)stream));
    if (!env_mask_dev) {
        e->was_reset = true; e->selection.masks_stale = false;
        if (!e->dev_tick) {      // nothing is finished any more: the lists of a batched-reset interval in progress are void
            HIP_TRY(hipMemsetAsync(e->g.done_count, 0, 2 * sizeof(int32_t), (hipStream_t)stream));
            e->steps_since_reset = 0; e->pending_interval = 0;
        }
        MATE_TRY(clear_message_tags(e, (hipStream_t)stream));
    }
    return attached_behind_new_records(e, (hipStream_t)stream);
}

// reset() with every random draw taken from a tape recorded from the reference (parity runs).
extern "C" int mate_engine_reset_tape(mate_engine *e, const uint8_t *env_mask_dev, const mate_step_io *io, const double *tape_dev,
                                      int32_t tape_len, int32_t *draws_used_dev, void *stream) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    MATE_TRY(enter(e, (hipStream_t)stream));
    if (!tape_dev || tape_len < 1) return fail(MATE_EINVAL, "reset_tape needs a tape");
    Ptrs g = e->g;
    apply_io(g, io);
    g.tape_goal = nullptr;                  // io->tape_camera_target_dev: see-through uniforms of the first view
    g.reset_mask = env_mask_dev;
    g.reset_tape = tape_dev; g.reset_tape_len = tape_len; g.reset_draws = draws_used_dev;
    MATE_TRY(launch_reset(e, g, env_mask_dev ? RESET_MASK : RESET_ALL, PH_PLACE | PH_LUT | PH_VIEW, (hipStream_t)stream));
    if (!env_mask_dev) { e->was_reset = true; e->selection.masks_stale = false; MATE_TRY(clear_message_tags(e, (hipStream_t)stream)); }
    return attached_behind_new_records(e, (hipStream_t)stream);
}

extern "C" int mate_engine_rebuild_luts(mate_engine *e, void *stream) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    MATE_TRY(enter(e, (hipStream_t)stream));
    return launch_reset(e, restart_ptrs(e), RESET_ALL, PH_LUT, (hipStream_t)stream);
}

extern "C" int mate_engine_set_episode_stats(mate_engine *e, double *stats_dev) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    e->g.ep_stats = stats_dev;
    return MATE_OK;
}

namespace {
__global__ void stats_snapshot_kernel(const double *__restrict__ src, double *__restrict__ dst) { if (threadIdx.x < 5) dst[threadIdx.x] = src[threadIdx.x]; }
}  // namespace

// A snapshot of the episode-statistics accumulators, ordered on `stream` behind the launches enqueued so far: one 64-thread workgroup
// (3 us; a 40-byte hipMemcpyAsync between device buffers took 10+ on the boxes measured).  What a sharded job hands to its all-gather.
extern "C" int mate_engine_snapshot_episode_stats(mate_engine *e, double *dst_dev, void *stream) {
    if (!e || !dst_dev) return fail(MATE_EINVAL, "null argument");
    if (!e->g.ep_stats) return fail(MATE_ESTATE, "snapshot_episode_stats: no accumulators (mate_engine_set_episode_stats)");
    HIP_TRY(hipSetDevice(e->device));
    hipLaunchKernelGGL(stats_snapshot_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double *)e->g.ep_stats, dst_dev);
    HIP_TRY(hipGetLastError());
    return MATE_OK;
}

// A batched-reset interval (auto_reset = k > 1) is in progress and the caller changes the mode: restart what has finished
// so far now, by flag, and forget the lists.
// `auto_reset`, `flow_tag`: of the call that is about to run -- an interval belongs to one k and one flow (kStepFlow / kRolloutFlow).
// It delivers NO first rows (mate_engine_enable_first_rows): it runs at the head of a later call, whose own frames then overwrite the rows.
constexpr int kStepFlow = 0x10000, kRolloutFlow = 0x20000;
static int flush_pending(mate_engine *e, int auto_reset, int flow_tag, hipStream_t stream) {
    if (e->steps_since_reset == 0 || (auto_reset > 1 ? (auto_reset | flow_tag) : auto_reset) == e->pending_interval) return MATE_OK;
    if (e->dev_tick) return fail(MATE_ESTATE, "auto_reset changed inside a reset interval while the step counter is device-resident");
    MATE_TRY(launch_reset(e, restart_ptrs(e), RESET_FLAGGED, PH_PLACE | PH_LUT | PH_VIEW, stream));
    HIP_TRY(hipMemsetAsync(e->g.done_count, 0, 2 * sizeof(int32_t), stream));
    e->steps_since_reset = 0; e->pending_interval = 0;
    return attached_behind_restart(e, stream);
}

// Device-resident step counter: see Params::dev_tick.  enable = k >= 1: the host's tick goes to the device and stays there,
// every step() must use auto_reset = k; disable: the stream is drained and the counter comes back.
// Leaving the pipelined-restart mode (any other entry point): the caller's stream waits for the resets still in flight on the
// side stream, and the "restarted" tags in the records become plain live environments.
static int leave_pipelined(mate_engine *e, hipStream_t stream) {
    if (!e->pipelined) return MATE_OK;
    HIP_TRY(hipSetDevice(e->device));
    for (int q = 0; q < 2; ++q)
        if (e->reset_in_flight[q]) { HIP_TRY(hipStreamWaitEvent(stream, e->ev_reset[q], 0)); e->reset_in_flight[q] = false; }
    if (e->pipe_count > 0) {         // an interval left open (restarts behind every pipe_every-th launch): what it has listed restarts now
        Ptrs r = restart_ptrs(e);
        r.pipelined = 1;
        MATE_TRY(launch_reset(e, r, RESET_DONE, PH_PLACE | PH_LUT | PH_VIEW, stream, true));
        HIP_TRY(hipMemsetAsync(e->g.done_count + e->parity, 0, sizeof(int32_t), stream));
        e->parity ^= 1;
        e->pipe_count = 0;
    }
    hipLaunchKernelGGL(untag_kernel, dim3((unsigned)((e->N + 255) / 256)), dim3(256), 0, stream, (const Params *)e->d_params, (const Ptrs)e->g);
    HIP_TRY(hipGetLastError());
    e->pipelined = false;
    note_stream(e, stream);
    return MATE_OK;
}
// Entering the mode (a call inside it changes nothing): the side stream and the events exist, both lists are empty, nothing is in flight.
static int enter_pipelined(mate_engine *e, int pipe_every, hipStream_t stream) {
    if (!e->side) {
        {   // the LOWEST priority the device offers (MATE_PIPELINED_PRIORITY=0: default priority): the resets' latency-bound workgroups
            // should take the slots the rollout launch leaves free -- its tail --, not displace its workgroups
            int least = 0, greatest = 0;
            HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
            if (!e->sw.pipelined_low_priority) HIP_TRY(hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking));
            else HIP_TRY(hipStreamCreateWithPriority(&e->side, hipStreamNonBlocking, least));
        }
        HIP_TRY(hipEventCreateWithFlags(&e->ev_launch, hipEventDisableTiming));
        for (int q = 0; q < 2; ++q) HIP_TRY(hipEventCreateWithFlags(&e->ev_reset[q], hipEventDisableTiming));
    }
    if (!e->pipelined) {
        HIP_TRY(hipMemsetAsync(e->g.done_count, 0, 2 * sizeof(int32_t), stream));
        e->reset_in_flight[0] = e->reset_in_flight[1] = false;
        e->pipelined = true;
        e->pipe_every = pipe_every; e->pipe_count = 0;
    }
    return MATE_OK;
}
// Behind a rollout launch of the mode, every pipe_every-th one: the reset of what this interval of launches finished (list `parity`) on the side
// stream, behind the launch and under the next ones.  Inside an interval the following launches append to the same list; what has finished idles
// (listed) until the interval's restart.
static int pipelined_restart(mate_engine *e, hipStream_t stream) {
    if (++e->pipe_count < e->pipe_every) return MATE_OK;
    e->pipe_count = 0;
    const bool serial = e->sw.pipelined_serial;
    hipStream_t rs = serial ? stream : e->side;
    if (!serial) { HIP_TRY(hipEventRecord(e->ev_launch, stream)); HIP_TRY(hipStreamWaitEvent(rs, e->ev_launch, 0)); }
    Ptrs r = restart_ptrs(e);
    r.pipelined = 1;
    const bool multi_before = e->multi_stream;
    MATE_TRY(launch_reset(e, r, RESET_DONE, PH_PLACE | PH_LUT | PH_VIEW, rs, true));
    HIP_TRY(hipMemsetAsync(e->g.done_count + e->parity, 0, sizeof(int32_t), rs));      // (the list is consumed: the launch after next appends to it afresh)
    if (!serial) { HIP_TRY(hipEventRecord(e->ev_reset[e->parity], rs)); e->reset_in_flight[e->parity] = true; }
    // (launch_reset noted the side stream: the accessors order it through leave_pipelined's event waits, so it neither becomes
    // the stream they wait for nor counts as a second stream of the CALLER's -- which would turn every accessor into a device-wide wait)
    e->last_stream = stream; e->multi_stream = multi_before;
    e->parity ^= 1;
    return MATE_OK;
}

extern "C" int mate_engine_device_tick(mate_engine *e, int32_t enable, void *stream_) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    hipStream_t stream = (hipStream_t)stream_;
    MATE_TRY(enter(e, stream));
    note_stream(e, stream);
    if ((enable != 0) == e->dev_tick && (!enable || enable == e->dev_interval)) return MATE_OK;
    if (enable && e->dev_tick) return fail(MATE_ESTATE, "device_tick: already enabled with interval %d", e->dev_interval);
    if (enable) MATE_TRY(flush_pending(e, 0, 0, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (enable) {
        e->p.dev_tick = e->tick; e->p.dev_group = (uint32_t)e->parity; e->p.dev_tick_on = 1;
        e->dev_interval = enable;
    } else {
        // The device counter holds the tick of the interval's first step; the steps of an interval that is still open
        // (the caller stopped between two reset launches) are added here, and what finished in it restarts now, by flag
        // (flush_pending, once the host counts again) -- the same thing a change of auto_reset inside an interval does.
        uint32_t words[2] = {0, 0};
        HIP_TRY(hipMemcpy(words, reinterpret_cast<const char *>(e->d_params) + offsetof(Params, dev_tick), sizeof(words), hipMemcpyDeviceToHost));
        e->tick = words[0] + (uint32_t)e->steps_since_reset * (uint32_t)e->dev_frames; e->parity = (int)(words[1] & 1u);
        e->p.dev_tick = 0; e->p.dev_group = 0; e->p.dev_tick_on = 0;      // zero while the host counts (the kernels ADD them to the launch arguments)
    }
    HIP_TRY(hipMemcpy(e->d_params, &e->p, sizeof(Params), hipMemcpyHostToDevice));
    e->dev_tick = enable != 0;
    if (enable) return MATE_OK;
    const int rc = flush_pending(e, 0, 0, stream);      // (an open interval's finished environments restart here)
    return attached_last(e, rc, stream);
}

// Device-resident step counter: the auto-reset launch advances it, so every stepping call uses the interval it was enabled with, and
// the launches of one reset interval all run the same number of frames (1: the per-step flows; K: FrameSkip launches).
// `one_frame_call`: step() and its kin, whose message names the mismatch from their side.
static int check_device_tick(mate_engine *e, int auto_reset, int frames, bool one_frame_call) {
    if (!e->dev_tick) return MATE_OK;
    if (auto_reset != e->dev_interval)
        return fail(MATE_ESTATE, "with a device-resident step counter (mate_engine_device_tick) step() needs auto_reset = %d: the auto-reset launch advances it", e->dev_interval);
    if (e->steps_since_reset == 0) e->dev_frames = frames;
    else if (e->dev_frames != frames)
        return one_frame_call ? fail(MATE_ESTATE, "device-resident step counter: a one-frame step inside a reset interval of %d-frame launches", e->dev_frames)
                              : fail(MATE_ESTATE, "device-resident step counter: %d frames per launch inside a reset interval that began with %d", frames, e->dev_frames);
    return MATE_OK;
}

// Behind a stepping launch: restart what has finished.  auto_reset = 1: now (list `parity`, which the launch appended to);
// k > 1: the finished environments idle, and the k-th launch of the interval restarts them together.  0 (or less): nothing.
// What differs between the flows is spelled by the caller:
struct Restart {
    const mate_step_io *io;      // the restart writes first observations and masks here (restart_ptrs); null: state only
    bool keep_actions;           // ... with the call's action pointers and encoding still in the record pointers
    int kind_batched;            // the interval's restart: RESET_DONE (by the lists: the per-step flows) or RESET_FLAGGED (the fused rollouts); immediate: RESET_DONE
    int phases;
    bool split_immediate, split_batched;   // launch_reset's split_done: a list-driven restart as placement / tables / view launches
    uint32_t frames;             // steps per launch: the restart advances a device-resident counter by frames * auto_reset (0: the flow has none)
    int flow_tag;                // kStepFlow / kRolloutFlow
    int fused_team = -1;         // the call is mate_engine_rollout_versus_greedy for this team (plan_attached: its restart may carry the first rows)
};
static int restart_finished(mate_engine *e, int auto_reset, const Restart &how, hipStream_t stream) {
    if (auto_reset < 1) return MATE_OK;
    const bool batched = auto_reset > 1;
    if (batched) {
        e->pending_interval = auto_reset | how.flow_tag;
        if (++e->steps_since_reset < auto_reset) return MATE_OK;
    }
    e->steps_since_reset = 0; e->pending_interval = 0;
    e->frames.closing = e->frames.in_call;      // (the restart of the call that has just enqueued its frame: the interval closes)
    Ptrs r = restart_ptrs(e, how.io);
    if (!how.keep_actions) { r.cam_act = r.tgt_act = nullptr; r.act_f64 = 0; r.act_discrete = 0; }
    if (plan_attached(e, false, how.fused_team).first_rows) {      // (the view launch computes the first view and packs it anyway: now it also stores -- the learner team's rows, its own record)
        (e->fragment.args.team == MATE_TEAM_CAMERA ? r.cam_obs : r.tgt_obs) = e->first.rows;
        r.scalars = e->first.scalars;
    }
    r.tick_advance = how.frames * (uint32_t)auto_reset;
    const int kind = batched ? how.kind_batched : RESET_DONE;
    MATE_TRY(launch_reset(e, r, kind, how.phases, stream, batched ? how.split_batched : how.split_immediate));
    if (kind == RESET_DONE && !e->dev_tick) e->parity ^= 1;      // (the list is consumed: the next launches append to the other one)
    return attached_behind_restart(e, stream, how.fused_team);      // (new episodes: their first rows; their goals are what the next step's sparse_delivery compares with)
}

// The per-step launch and what follows it, behind the state checks of the call: launch_step's, or those step_with_policies makes ahead of its agents' launch
static int step_launches(mate_engine *e, const mate_step_io *io, int mode, int auto_reset, hipStream_t stream, bool selected) {
    note_stream(e, stream);
    if (mode != MODE_OBSERVE) MATE_TRY(flush_pending(e, auto_reset, kStepFlow, stream));
    Ptrs g = e->g;
    apply_io(g, io);
    if (e->greedy_team_bits) g.act_f64 |= e->greedy_team_bits;          // the on-device agents' team(s): f64 joint actions
    if (mode == MODE_STEP && ((e->p.Nc > 0 && !g.cam_act) || !g.tgt_act)) return fail(MATE_EINVAL, "step() needs camera and target joint actions");
    if (mode == MODE_STEP && (((g.act_discrete & 1) && !g.cam_grid) || ((g.act_discrete & 2) && !g.tgt_grid)))
        return fail(MATE_ESTATE, "discrete actions passed before mate_engine_set_action_grids");
    g.mode = mode; g.parity = e->dev_tick ? 0 : e->parity; g.reset_kind = -1;
    g.tick = e->dev_tick ? (uint32_t)e->steps_since_reset : e->tick;     // device-resident counter: the offset inside the reset interval
    // auto_reset = 1: finished environments restart inside this call; k > 1: they idle (listed for it) and restart together every k-th call
    g.freeze_done = auto_reset > 1;
    if (mode == MODE_OBSERVE || auto_reset == 0) g.done_count = nullptr;
    Timed t;
    MATE_TRY(take_timing_events(e, !e->dev_tick && mode != MODE_OBSERVE, &t));
    const LaunchPlan pl = plan_step(e, mode, g);
    e->last_flow = pl.last_flow;
    if (pl.E > 1) { g.per_step = 1; g.rollout_steps = 1; g.rotate_prio = 0; }      // (the sub-wave rollout kernel with ONE step)
    if (mode != MODE_OBSERVE) MATE_TRY(launch_trace(e, g.freeze_done, stream));      // (2d: behind the agents' launches, ahead of the step)
    launch(pl.step, dim3(pl.blocks), dim3(pl.threads), pl.lds, stream, t, e->d_params, g);
    HIP_TRY(hipGetLastError());
    e->selection.masks_stale = false;
    if (mode == MODE_OBSERVE) return MATE_OK;
    if (!e->dev_tick) e->tick += 1;
    MATE_TRY(attached_behind_step(e, selected, io, 1, stream));      // (the finished step's rows, the terminal one included: ahead of the restart)
    // (the restart writes the caller's observation buffers and masks; the immediate one, idle almost always, stays ONE launch, and so
    // does the interval's unless the on-device agents play: their ~1.2 k-step episodes finish somewhere in the batch all the time)
    return restart_finished(e, auto_reset, Restart{io, true, RESET_DONE, PH_PLACE | PH_LUT | PH_VIEW, false, e->greedy_team_bits != 0, 1u, kStepFlow}, stream);
}

static int launch_step(mate_engine *e, const mate_step_io *io, int mode, int auto_reset, hipStream_t stream) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    MATE_TRY(enter(e, stream, "step()/observe()"));
    if (mode != MODE_OBSERVE) MATE_TRY(check_device_tick(e, auto_reset, 1, true));
    if (mode != MODE_OBSERVE) MATE_TRY(check_attached_call(e, io, false, false));
    return step_launches(e, io, mode, auto_reset, stream, false);
}

extern "C" int mate_engine_step(mate_engine *e, const mate_step_io *io, int32_t auto_reset, void *stream) {
    return attached_last(e, launch_step(e, io, MODE_STEP, auto_reset, (hipStream_t)stream), (hipStream_t)stream);
}
extern "C" int mate_engine_step_random(mate_engine *e, const mate_step_io *io, int32_t auto_reset, void *stream) {
    return attached_last(e, launch_step(e, io, MODE_STEP_RANDOM, auto_reset, (hipStream_t)stream), (hipStream_t)stream);
}
// The fused K-frame launches never materialise their frames' edges: refused while a communication trace is enabled, as under a channel
static int refuse_traced_rollout(const mate_engine *e, const char *who) {
    return e->trace.on() ? fail(MATE_ESTATE, "%s: a communication trace is enabled (mate_engine_enable_comm_trace) and the fused launches keep no per-frame edges: step per frame, or detach the trace", who) : MATE_OK;
}
static int rollout_random_impl(mate_engine *e, const mate_step_io *io, int32_t steps, int32_t auto_reset, void *stream_) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    hipStream_t stream = (hipStream_t)stream_;
    MATE_TRY(refuse_traced_rollout(e, "rollout_random"));
    MATE_TRY(enter(e, stream, "rollout"));
    if (e->dev_tick) return fail(MATE_ESTATE, "not available while the step counter is device-resident (mate_engine_device_tick)");
    if (steps < 1) return fail(MATE_EINVAL, "rollout needs at least one step");
    MATE_TRY(check_attached_call(e, io, false, false));
    note_stream(e, stream);
    MATE_TRY(flush_pending(e, auto_reset, kRolloutFlow, stream));
    Ptrs g = e->g;
    apply_io(g, io);
    g.mode = MODE_STEP_RANDOM; g.parity = e->parity; g.reset_kind = -1; g.tick = e->tick; g.rollout_steps = steps;
    g.tape_ct = nullptr; g.tape_goal = nullptr;
    g.rotate_prio = e->sw.rollout_rotate;
    if (auto_reset != 1) g.done_count = nullptr;     // no list: nothing restarts (0), or a batched reset finds the finished ones by their flag (k > 1)
    Timed t;
    MATE_TRY(take_timing_events(e, true, &t));
    const LaunchPlan pl = plan_rollout_random(e, g);
    e->last_flow = pl.last_flow;
    // (this flow has always gone through the extended launch, timed or not -- null events: not through launch())
    hipExtLaunchKernelGGL(pl.step, dim3(pl.blocks), dim3(pl.threads), pl.lds, stream, t.a, t.b, 0, (const Params *)e->d_params, (const Ptrs)g);
    HIP_TRY(hipGetLastError());
    e->tick += (uint32_t)steps;
    MATE_TRY(attached_behind_step(e, false, io, steps, stream));
    // (state only, placement and tables: the next rollout observes the fresh episode on its first step)
    if (auto_reset >= 1) e->selection.masks_stale = true;      // (... and until then the view masks of a restarted environment are its finished episode's)
    return restart_finished(e, auto_reset, Restart{nullptr, false, RESET_FLAGGED, PH_PLACE | PH_LUT, false, false, 0u, kRolloutFlow}, stream);
}

extern "C" int mate_engine_rollout_random(mate_engine *e, const mate_step_io *io, int32_t steps, int32_t auto_reset, void *stream) {
    return attached_last(e, rollout_random_impl(e, io, steps, auto_reset, stream), (hipStream_t)stream);      // (the state after the launch's last frame)
}

static int policy_enable(mate_engine *e) {
    if (e->policy_ready) return MATE_OK;
    const Params &p = e->p;
    PolicyPtrs &q = e->q;
    q.TW = pol_target_words(p.Nt);
    q.PW = pol_record_words(p.Nc, p.Nt);
    q.caller_team = -1;
    q.memory_period = 25;      // greedy.py:21
    q.noise_scale = 0.5;       // greedy.py:236
    q.lds_bytes = round_up((q.PW + policy_staging_words(p.Nc, p.Nt) + p.SW + p.DW) * 8 + p.MW * 4 + 4, 16);   // (+ one mask word of slack: seen_mask reads two)
    MATE_TRY(dev_alloc(e, &q.pol, (size_t)e->N * q.PW));
    MATE_TRY(dev_alloc(e, &q.cam_act, (size_t)e->N * std::max(p.Nc, 1) * 2));
    MATE_TRY(dev_alloc(e, &q.tgt_act, (size_t)e->N * p.Nt * 2));
    if (!e->g.own_masks) MATE_TRY(dev_alloc(e, &e->g.own_masks, (size_t)e->N * p.MW));
    q.masks = e->g.own_masks;
    {   // GreedyCameraAgent's zoom solve (greedy.py:139-145) as a function of K = area_product / distance^2 alone, tabulated with the
        // reference's own iteration (policy_kernels.hpp: zoom_lookup interpolates it to 1.5e-13)
        constexpr double kInvH = 40.0, kMaxK = 720.0;
        // (the last node is K = 720 itself: beyond it the clamp of the half angle at 90 degrees kinks the function, and a stencil
        // that reaches across the kink was off by 2e-8 degrees for K in (719.95, 720); zoom_lookup iterates where its four
        // nodes are not all inside the table)
        const int n = (int)(kMaxK * kInvH) + 1;
        std::vector<double> tab((size_t)n);
        for (int i = 0; i < n; ++i) {
            const double K = (double)i / kInvH;
            double b = 180.0;
            for (int it = 0; it < 20; ++it) {
                const double half = b * 0.5;
                const double y = 1.0 + std::sin((half < 90.0 ? half : 90.0) * (3.14159265358979323846 / 180.0));
                b = K / (y * y);
            }
            tab[(size_t)i] = b;
        }
        double *d_tab = nullptr;
        MATE_TRY(dev_alloc(e, &d_tab, (size_t)n, false));
        HIP_TRY(hipMemcpy(d_tab, tab.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
        q.zoom_tab = d_tab; q.zoom_inv_h = kInvH; q.zoom_n = e->sw.zoom_iterate ? 0 : n;      // 0 entries: zoom_lookup iterates
    }
    // dynamic LDS of the agents' kernel and of everything plan_with_policies can return for this engine: the forms that fit a workgroup
    hipError_t err = set_dynamic_lds(e->k.policy, 4 * (size_t)q.lds_bytes + 1024);
    for (int form = 0; form < kPolicyForms; ++form) {
        const LaunchPlan pl = policy_form(e, form, -1);      // (-1: step_greedy_kernel's larger workgroup, both teams' agents)
        if (err == hipSuccess && pl.fits()) err = set_dynamic_lds(pl.policy, pl.lds);
    }
    if (err != hipSuccess) return fail(MATE_EHIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(err));
    e->policy_ready = true;
    return MATE_OK;
}

// Turn on the engine-owned mask copy the on-device policies read (must precede the reset / step whose view they act on).
extern "C" int mate_engine_policy_enable(mate_engine *e) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    return policy_enable(e);
}

// What a call brings for the ONE-launch form with the on-device agents.  Both gates of that form read THIS: rollout_with_policies turns the first one
// missing into its error; step_with_policies runs its two-launch form instead, whose checks then name what is wrong with the call itself.
struct FusedCall {
    bool reset, ready;      // an episode is in progress; mate_engine_policy_enable has run
    bool outputs, plain;    // every observation and scalar output is there; no fused observation transform / team mode
    bool action;            // the caller's team (if any) brought its joint action
    bool complete() const { return reset && ready && outputs && plain && action; }
};
static FusedCall fused_call(const mate_engine *e, int team_caller, const mate_step_io *io) {
    return {e->was_reset, e->policy_ready, io && (io->camera_obs_dev || e->p.Nc == 0) && io->target_obs_dev && io->scalars_dev,
            e->g.obs_mode == 0 && !e->g.xdesc, team_caller < 0 || (io && (team_caller == 0 ? io->camera_actions_dev : io->target_actions_dev))};
}
// step_greedy / step_versus_greedy as one launch: a complete call, and nothing that only the two-launch form serves -- MATE_POLICY_SPLIT=1,
// recorded agent draws, tapes of the step itself, f64 observations, the Heuristic target opponent (its drift launch sits between the two),
// the Heuristic camera opponent (its launch takes the camera agents' place), an opponent mixture whose rows come from the scripted launch,
// a communication channel of a team whose talking agents act (greedy_channel_kernel is the agents' launch then): OpponentPlan::one_launch
static bool one_launch_step(const mate_engine *e, const FusedCall &c, const OpponentPlan &op, const mate_step_io *io, const mate_policy_tape *tape) {
    return c.complete() && !e->sw.policy_split && !tape && !io->tape_camera_target_dev && !io->tape_goal_dev && !e->p.obs_f64 && op.one_launch;
}
#include "opponent_host.inc"      // the opponents' launches, setters and accessors
#include "message_host.inc"       // the learner's own messages: enable, the routing launch, draws, accessors
#include "frame_host.inc"         // the per-frame FrameSkip fragments: enable, the call's check, the on-demand launch
#include "render_host.inc"        // the off-screen render: the argument check, the launch
#include "trace_host.inc"         // the communication trace: enable, the one launch of a stepping call, the accessor

static int rollout_with_policies(mate_engine *e, int team_caller, const mate_step_io *io, int32_t steps, int32_t auto_reset, void *stream_, bool per_step = false, bool selected = false);

// team_caller: -1 = both teams are the on-device agents; 0 / 1 = the camera / target team's joint action is the caller's
// selected: the call is mate_engine_step_selected (the camera team's joint action is the executor's; the metrics follow the step)
static int step_with_policies(mate_engine *e, int team_caller, const mate_step_io *io, const mate_policy_tape *tape, int32_t auto_reset, hipStream_t stream, bool selected = false) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    // (pipelined restarts still in flight rewrite records, masks and `done` tags on the side stream: the agents' kernel of the
    // two-launch form reads all three, so the mode is left HERE, not only in launch_step behind it)
    MATE_TRY(leave_pipelined(e, stream));
    if (!selected) MATE_TRY(check_attached_call(e, io, false, false));      // (ahead of the agents' launch: a rejected call leaves their memory alone; step_selected has made it)
    const FusedCall c = fused_call(e, team_caller, io);
    const OpponentPlan op = plan_opponents(e, team_caller);
    if (one_launch_step(e, c, op, io, tape) && plan_with_policies(e, true, team_caller).fits())
        return rollout_with_policies(e, team_caller, io, 1, auto_reset, (void *)stream, true, selected);
    if (!c.reset) return fail(MATE_ESTATE, "step_greedy called before reset() (or import_state)");
    // (works with a device-resident step counter too -- the agents take their tick from the environment record -- so the
    // learner-versus-greedy loop can be captured in a HIP graph like step(); launch_step checks the reset interval)
    if (!c.ready) return fail(MATE_ESTATE, "call mate_engine_policy_enable() before the reset whose observations the policies act on");
    if (team_caller == 0 && e->p.Nc == 0) return fail(MATE_EINVAL, "the scenario has no cameras to act for");
    if (!c.action) return fail(MATE_EINVAL, "step_versus_greedy needs the %s team's joint action", team_caller == 0 ? "camera" : "target");
    // (with the checks above, everything launch_step checks: made here, ahead of the policy launch that advances the agents' memory -- a rejected call must leave it alone)
    MATE_TRY(check_device_tick(e, auto_reset, 1, true));
    HIP_TRY(hipSetDevice(e->device));
    note_stream(e, stream);
    PolicyPtrs q = e->q;
    std::memset(&q.tape, 0, sizeof(q.tape));
    q.caller_team = op.caller_team;      // (the agents of that team do not act: greedy_policy_body)
    if (tape) {
        q.tape.cam_binom_u = tape->camera_resample_u_dev; q.tape.cam_sample_u = tape->camera_sample_u_dev;
        q.tape.cam_delay = tape->camera_delay_dev; q.tape.tgt_choice_u = tape->target_choice_u_dev;
        q.tape.tgt_binom_u = tape->target_resample_u_dev; q.tape.tgt_sample_u = tape->target_sample_u_dev;
        q.tape.tgt_reset_sample_u = tape->target_reset_sample_u_dev;
    }
    const unsigned blocks = (unsigned)((e->N + 3) / 4);
    Ptrs gp = e->g;
    gp.freeze_done = auto_reset > 1;
    // the launches in the order of the plan's fields: the agents', the Heuristic cameras', the drift, the scripted one; then whose rows the step consumes
    if (op.channel_kernel) {      // the channel inside the agents' `communicate` phase (channel_rows.hpp)
        HIP_TRY(launch_greedy_channel(e->p.obs_f64 != 0, blocks, 4 * (size_t)e->channel.lds_bytes, stream, e->d_params, gp, q, channel_args(e, op)));
    } else if (op.agents) {
        launch(e->k.policy, dim3(blocks), dim3(256), 4 * q.lds_bytes + 1024, stream, Timed{}, e->d_params, gp, q);   // + the shared zoom-solve exchange
        HIP_TRY(hipGetLastError());
    }
    if (op.team[MATE_TEAM_CAMERA].heuristic) MATE_TRY(launch_heuristic_cameras(e, tape, gp.freeze_done, stream));
    if (op.team[MATE_TEAM_TARGET].heuristic) MATE_TRY(launch_drift(e, op, gp.freeze_done, stream));
    if (op.team[MATE_TEAM_CAMERA].scripted || op.team[MATE_TEAM_TARGET].scripted) MATE_TRY(launch_scripted(e, op, gp.freeze_done, stream));
    mate_step_io io2;
    if (io) io2 = *io; else std::memset(&io2, 0, sizeof(io2));
    // the caller's team keeps its own pointer and encoding (f32 / f64 / grid indices); the agents' joint action is f64 pairs
    if (team_caller != MATE_TEAM_CAMERA) { io2.camera_actions_dev = rows_of(e, MATE_TEAM_CAMERA, op.team[MATE_TEAM_CAMERA].source); io2.act_dtype &= ~MATE_ACT_CAMERA_DISCRETE; }
    if (team_caller != MATE_TEAM_TARGET) { io2.target_actions_dev = rows_of(e, MATE_TEAM_TARGET, op.team[MATE_TEAM_TARGET].source); io2.act_dtype &= ~MATE_ACT_TARGET_DISCRETE; }
    for (int team = 0; team < 2; ++team) e->opponents.consumed[team] = op.team[team].source;
    e->greedy_team_bits = team_caller < 0 ? 3 : (team_caller == 0 ? 2 : 1);
    // (greedy_channel_kernel writes the edges of every team that acts in it -- OpponentPlan::Team::greedy: the team's Greedy agents run in the agents' launch, as the
    // team's players or for a mixture that has a Greedy candidate, or Heuristic targets built on them; a team of Naive / Random agents alone is not in that launch and sends nothing)
    for (int team = 0; team < 2; ++team) e->trace.team[team].call_delivered = op.channel_kernel && op.team[team].greedy;
    const int rc = step_launches(e, &io2, MODE_STEP, auto_reset, stream, selected);
    for (int team = 0; team < 2; ++team) e->trace.team[team].call_delivered = false;
    e->greedy_team_bits = 0;
    return rc;
}

extern "C" int mate_engine_step_greedy(mate_engine *e, const mate_step_io *io, const mate_policy_tape *tape, int32_t auto_reset, void *stream) {
    return attached_last(e, step_with_policies(e, -1, io, tape, auto_reset, (hipStream_t)stream), (hipStream_t)stream);
}

extern "C" int mate_engine_step_versus_greedy(mate_engine *e, int32_t team, const mate_step_io *io, const mate_policy_tape *tape, int32_t auto_reset, void *stream) {
    if (team != MATE_TEAM_CAMERA && team != MATE_TEAM_TARGET) return fail(MATE_EINVAL, "team must be MATE_TEAM_CAMERA or MATE_TEAM_TARGET");
    if (e && e->frames.on && e->frames.team == team) {      // (the call enqueues the frame launch: plan_attached reads in_call / closing while it runs)
        MATE_TRY(check_frame_call(e, io, auto_reset));
        e->frames.in_call = true; e->frames.closing = false;
    }
    const int rc = attached_last(e, step_with_policies(e, team, io, tape, auto_reset, (hipStream_t)stream), (hipStream_t)stream);
    if (e) e->frames.in_call = e->frames.closing = false;
    return rc;
}

// The learner's seat among on-device teammates (include/mate_engine.h, csrc/seat_rows.hpp): step_with_policies' two-launch form with both teams the engine's,
// greedy_seat_kernel as the agents' launch and the seat's action from the seat team's pointer of `io`; what the OTHER team's plan adds, in plan_opponents' order;
// the stepping launch on both teams' engine-owned rows; the attached observers and the restart as for step_greedy.  Identical arguments at every call but for
// the tapes, no allocation, no synchronisation.
static int step_seated(mate_engine *e, const mate_step_io *io, const mate_policy_tape *tape, int32_t auto_reset, hipStream_t stream) {
    MATE_TRY(leave_pipelined(e, stream));
    if (!e->policy_ready) return fail(MATE_ESTATE, "step_seated: call mate_engine_policy_enable() before the reset whose observations the policies act on");
    const Seat &s = e->seat;
    if (!s.on) return fail(MATE_ESTATE, "step_seated: call mate_engine_enable_seat() first");
    const int team = s.spec.team;
    const OpponentPlan op = plan_opponents(e, -1, team);
    if (op.seat_refusal != SEAT_OK) return fail(MATE_ESTATE, "step_seated (%s team): %s", kTeamNames[team], seat_refusal_text(op.seat_refusal));
    MATE_TRY(check_attached_call(e, io, false, false));      // (ahead of the agents' launch: a rejected call leaves their memory alone)
    if (!e->was_reset) return fail(MATE_ESTATE, "step_seated called before reset() (or import_state)");
    if (!io || !(team == MATE_TEAM_CAMERA ? io->camera_actions_dev : io->target_actions_dev)) return fail(MATE_EINVAL, "step_seated needs the seat's action in the %s team's action pointer", kTeamNames[team]);
    if (!(team == MATE_TEAM_CAMERA ? io->camera_obs_dev : io->target_obs_dev)) return fail(MATE_EINVAL, "step_seated needs the %s team's observation output (the seat's row is gathered from it)", kTeamNames[team]);
    if ((io->act_dtype & (team == MATE_TEAM_CAMERA ? MATE_ACT_CAMERA_DISCRETE : MATE_ACT_TARGET_DISCRETE)) && !(team == MATE_TEAM_CAMERA ? e->g.cam_grid : e->g.tgt_grid))
        return fail(MATE_ESTATE, "discrete actions passed before mate_engine_set_action_grids");
    MATE_TRY(check_device_tick(e, auto_reset, 1, true));
    HIP_TRY(hipSetDevice(e->device));
    note_stream(e, stream);
    PolicyPtrs q = e->q;
    std::memset(&q.tape, 0, sizeof(q.tape));
    q.caller_team = op.caller_team;      // (an opposing team other launches play sits out)
    if (tape) {
        q.tape.cam_binom_u = tape->camera_resample_u_dev; q.tape.cam_sample_u = tape->camera_sample_u_dev;
        q.tape.cam_delay = tape->camera_delay_dev; q.tape.tgt_choice_u = tape->target_choice_u_dev;
        q.tape.tgt_binom_u = tape->target_resample_u_dev; q.tape.tgt_sample_u = tape->target_sample_u_dev;
        q.tape.tgt_reset_sample_u = tape->target_reset_sample_u_dev;
    }
    Ptrs gp = e->g;
    apply_io(gp, io);                    // (the seat's action: pointer, type, grid)
    gp.freeze_done = auto_reset > 1;
    HIP_TRY(launch_greedy_seat(e->p.obs_f64 != 0, blocks_of(e, 4), 4 * (size_t)q.lds_bytes, stream, e->d_params, gp, q, SeatArgs{s.spec, s.acted, s.d_live}));
    if (op.team[MATE_TEAM_CAMERA].heuristic) MATE_TRY(launch_heuristic_cameras(e, tape, gp.freeze_done, stream));
    if (op.team[MATE_TEAM_TARGET].heuristic) MATE_TRY(launch_drift(e, op, gp.freeze_done, stream));
    if (op.team[MATE_TEAM_CAMERA].scripted || op.team[MATE_TEAM_TARGET].scripted) MATE_TRY(launch_scripted(e, op, gp.freeze_done, stream));
    mate_step_io io2 = *io;
    io2.camera_actions_dev = rows_of(e, MATE_TEAM_CAMERA, op.team[MATE_TEAM_CAMERA].source);
    io2.target_actions_dev = rows_of(e, MATE_TEAM_TARGET, op.team[MATE_TEAM_TARGET].source);
    io2.act_dtype &= ~(MATE_ACT_CAMERA_DISCRETE | MATE_ACT_TARGET_DISCRETE);
    for (int t = 0; t < 2; ++t) e->opponents.consumed[t] = op.team[t].source;
    e->greedy_team_bits = 3;
    const int rc = step_launches(e, &io2, MODE_STEP, auto_reset, stream, false);
    e->greedy_team_bits = 0;
    return rc;
}
extern "C" int mate_engine_step_seated(mate_engine *e, const mate_step_io *io, const mate_policy_tape *tape, int32_t auto_reset, void *stream) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    const int rc = attached_last(e, step_seated(e, io, tape, auto_reset, (hipStream_t)stream), (hipStream_t)stream);
    return rc == MATE_OK ? seat_rows_behind(e, io, true, (hipStream_t)stream) : rc;
}
extern "C" int mate_engine_seat_rows(mate_engine *e, const mate_step_io *io, void *stream) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (!e->seat.on) return fail(MATE_ESTATE, "seat_rows: call mate_engine_enable_seat() first");
    if (!e->was_reset) return fail(MATE_ESTATE, "seat_rows called before reset() (or import_state)");
    if (!io || !(e->seat.spec.team == MATE_TEAM_CAMERA ? io->camera_obs_dev : io->target_obs_dev)) return fail(MATE_EINVAL, "seat_rows needs the %s team's observation rows", kTeamNames[e->seat.spec.team]);
    MATE_TRY(enter(e, (hipStream_t)stream));
    note_stream(e, (hipStream_t)stream);
    return seat_rows_behind(e, io, false, (hipStream_t)stream);
}

// Target-selection camera actions (include/mate_engine.h).  The buffers are the caller's, but for the joint action the executor hands to
// the stepping launch: engine-owned, f64 unless MATE_SELECTION_ACT_F32.
extern "C" int mate_engine_enable_selection(mate_engine *e, int32_t mode, const void *selection_dev, double *metrics_dev, int32_t *frames_dev,
                                            uint8_t *action_mask_dev, int32_t flags) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (!selection_dev) return fail(MATE_EINVAL, "enable_selection: null selection buffer");
    if (mode != MATE_SELECTION_SINGLE && mode != MATE_SELECTION_MULTI) return fail(MATE_EINVAL, "enable_selection: mode must be MATE_SELECTION_SINGLE or MATE_SELECTION_MULTI");
    if (flags & ~(MATE_SELECTION_ACCUMULATE | MATE_SELECTION_ACT_F32)) return fail(MATE_EINVAL, "enable_selection: unknown flag bits");
    if (e->p.Nc == 0) return fail(MATE_EINVAL, "enable_selection: the scenario has no cameras to act for");
    if ((reinterpret_cast<uintptr_t>(selection_dev) & 3u) || (reinterpret_cast<uintptr_t>(metrics_dev) & 7u) || (reinterpret_cast<uintptr_t>(frames_dev) & 3u))
        return fail(MATE_EINVAL, "enable_selection: a buffer is not aligned to its element size");
    if (!e->policy_ready) return fail(MATE_ESTATE, "enable_selection: call mate_engine_policy_enable() first (the opponents, and the engine's own view masks)");
    if (!e->was_reset) return fail(MATE_ESTATE, "enable_selection called before reset() (or import_state)");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(wait_for_launches(e));      // (no launch reads the arguments while they change)
    if (!e->selection.d_actions) MATE_TRY(dev_alloc(e, &e->selection.d_actions, (size_t)e->N * e->p.Nc * 2));
    mate_layout layout;
    MATE_TRY(mate_engine_get_layout(e, &layout));
    SelectionArgs a{};
    a.selection = selection_dev; a.actions = e->selection.d_actions;
    a.metrics = metrics_dev; a.frames = frames_dev; a.action_mask = action_mask_dev;
    a.multi = mode == MATE_SELECTION_MULTI; a.accumulate = (flags & MATE_SELECTION_ACCUMULATE) != 0;
    a.bit_ct = layout.bit_camera_target;
    e->selection.args = a; e->selection.act_f64 = !(flags & MATE_SELECTION_ACT_F32);
    e->selection.on = true;
    const AttachedPlan pl = plan_attached(e, false);
    if (!pl.action_mask) return MATE_OK;
    // action_mask() of the observation rows as they are, complete when the call returns (the caller need not know the stream)
    MATE_TRY(launch_selection(e, pl, SELECTION_ACTION_MASK, nullptr, e->last_stream));
    HIP_TRY(hipStreamSynchronize(e->last_stream));
    return MATE_OK;
}
extern "C" int mate_engine_disable_selection(mate_engine *e) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    e->selection.on = false;
    return MATE_OK;
}
extern "C" int mate_engine_selection_actions(mate_engine *e, void **actions_dev, int32_t *act_dtype) {
    if (!e || !actions_dev) return fail(MATE_EINVAL, "null argument");
    if (!e->selection.on) return fail(MATE_ESTATE, "selection_actions: mate_engine_enable_selection has not run");
    *actions_dev = e->selection.d_actions;
    if (act_dtype) *act_dtype = e->selection.act_f64 ? MATE_ACT_F64 : MATE_ACT_F32;
    return MATE_OK;
}

// The attached launches around exactly what mate_engine_step_versus_greedy(team = camera) enqueues, with the engine-owned joint action.
extern "C" int mate_engine_step_selected(mate_engine *e, const mate_step_io *io, const mate_policy_tape *tape, int32_t auto_reset, void *stream_) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    hipStream_t stream = (hipStream_t)stream_;
    MATE_TRY(check_attached_call(e, io, false, true, auto_reset));
    MATE_TRY(check_device_tick(e, auto_reset, 1, true));      // (a rejected call launches nothing)
    // the state checks of the stepping flows and what they enqueue ahead of their launch, all AHEAD of the executor: a rejected call
    // leaves the action buffer alone; pipelined restarts in flight are joined before the executor reads the mask words; an open
    // reset interval of another flow restarts what it finished before the executor looks at it
    MATE_TRY(enter(e, stream, "step_selected"));
    if (!e->policy_ready) return fail(MATE_ESTATE, "step_selected: call mate_engine_policy_enable() before the reset whose observations the policies act on");
    note_stream(e, stream);
    MATE_TRY(flush_pending(e, auto_reset, kStepFlow, stream));
    mate_step_io io2 = *io;
    io2.camera_actions_dev = e->selection.d_actions;
    io2.act_dtype = (io->act_dtype & ~(0xff | MATE_ACT_CAMERA_DISCRETE)) | (e->selection.act_f64 ? MATE_ACT_F64 : MATE_ACT_F32);
    int rc = attached_ahead_of_step(e, true, stream);
    if (rc == MATE_OK) rc = step_with_policies(e, MATE_TEAM_CAMERA, &io2, tape, auto_reset, stream, true);
    return attached_last(e, rc, stream);
}

// What differs between the two forms of rollout_with_policies, spelled once (after struct Restart):
//   fused (rollout_greedy / rollout_versus_greedy): rollout-shaped outputs; restarts of state and the engine's own masks -- the agents of the next
//     rollout act on the fresh view --, the interval's by flag, so the finished-episode list exists for the immediate and the pipelined restart only;
//   per-step: ONE launch with the semantics of the per-step flows -- outputs in the caller's [N][...] buffers, immediate (auto_reset = 1) or batched
//     (k > 1: finished environments idle, listed, and restart together behind every k-th call) list-driven restarts that write the restarted
//     environments' first observations (not its actions' encoding; the immediate one, idle almost always, stays ONE launch, the interval's is split:
//     placement / tables / view), and the device-resident step counter (graph replay).  What step_greedy / step_versus_greedy run (one_launch_step).
struct PolicyFlow {
    Restart restart;             // (its flow_tag is the interval tag of flush_pending too)
    bool keep_list;              // this call's auto_reset restarts by the finished-episode list
    bool may_pipeline;           // auto_reset = MATE_RESET_PIPELINED
    bool may_count_on_device;    // mate_engine_device_tick: the per-step flows, and the K-frame launches of a learner against the greedy opponents --
                                 // FrameSkip in a HIP graph; the auto-reset launch behind every auto_reset-th launch advances the counter by auto_reset * K
};

// The fused K-frame launches hold the Greedy agents and deliver every message: the one refusal the opponents of the call give (OpponentPlan::refusal), `who` refusing
static int refuse_fused(const OpponentPlan &op, const char *who) {
    const char *team = op.refusal == FUSED_OK ? "" : kTeamNames[op.refusal_team];
    switch (op.refusal) {
    case FUSED_MIXTURE: return fail(MATE_ESTATE, "%s: the fused launches hold the Greedy agents, the %s team plays an opponent mixture (mate_engine_set_opponent_mixture): step per frame, or clear the mixture", who, team);
    case FUSED_CHANNEL: return fail(MATE_ESTATE, "%s: the fused launches deliver every message, a communication channel is set for the %s team (mate_engine_set_channel): step per frame, or clear the channel", who, team);
    case FUSED_HEURISTIC: return fail(MATE_ESTATE, "%s: the fused launches hold the Greedy agents, the %s opponent is the heuristic one (mate_engine_set_%s_opponent): step per frame, or select MATE_OPPONENT_GREEDY", who, team, team);
    default: return MATE_OK;
    }
}
static int rollout_with_policies(mate_engine *e, int team_caller, const mate_step_io *io, int32_t steps, int32_t auto_reset, void *stream_, bool per_step, bool selected) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    const FusedCall c = fused_call(e, team_caller, io);
    const bool pipelined = auto_reset < 0;          // MATE_RESET_PIPELINED (-1), or -m: one restart launch behind every m-th rollout launch
    const int full = PH_PLACE | PH_LUT | PH_VIEW;
    const PolicyFlow flow = per_step ? PolicyFlow{Restart{io, false, RESET_DONE, full, false, true, 1u, kStepFlow}, auto_reset != 0, false, true}
                                     : PolicyFlow{Restart{nullptr, false, RESET_FLAGGED, full, true, false, (uint32_t)steps, kRolloutFlow, team_caller}, auto_reset == 1 || pipelined, true, team_caller >= 0};
    if (!c.reset) return fail(MATE_ESTATE, "rollout_greedy called before reset() (or import_state)");
    if (!per_step) MATE_TRY(refuse_traced_rollout(e, team_caller < 0 ? "rollout_greedy" : "rollout_versus_greedy"));
    MATE_TRY(refuse_fused(plan_opponents(e, team_caller), team_caller < 0 ? "rollout_greedy" : "rollout_versus_greedy"));      // (a per-step call never arrives here with one: one_launch_step)
    if (e->dev_tick && !flow.may_count_on_device) return fail(MATE_ESTATE, "not available while the step counter is device-resident (mate_engine_device_tick)");
    MATE_TRY(check_device_tick(e, auto_reset, steps, false));
    if (!c.ready) return fail(MATE_ESTATE, "call mate_engine_policy_enable() before the reset whose observations the policies act on");
    if (steps < 1) return fail(MATE_EINVAL, "rollout needs at least one step");
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(e->device));
    if (auto_reset < -(1 << 16)) return fail(MATE_EINVAL, "auto_reset = %d: pipelined restarts every -auto_reset launches take 1 .. 65536", auto_reset);
    const int pipe_every = pipelined ? -auto_reset : 1;
    if (pipelined && (!flow.may_pipeline || e->dev_tick)) return fail(MATE_EINVAL, "pipelined restarts (auto_reset = MATE_RESET_PIPELINED) belong to the fused rollouts");
    if (!per_step) MATE_TRY(check_attached_call(e, io, pipelined, false, 0, team_caller));      // (per_step: step_with_policies has made it)
    if (!pipelined || (e->pipelined && e->pipe_every != pipe_every)) MATE_TRY(leave_pipelined(e, stream));
    note_stream(e, stream);
    MATE_TRY(flush_pending(e, auto_reset, flow.restart.flow_tag, stream));
    if (pipelined) MATE_TRY(enter_pipelined(e, pipe_every, stream));
    Ptrs g = e->g;
    apply_io(g, io);
    g.pipelined = pipelined ? 1 : 0;
    if (!c.outputs) return fail(MATE_EINVAL, "rollout_greedy needs the observation and scalar outputs");
    if (!c.plain) return fail(MATE_EINVAL, "rollout_greedy packs plain observations (no fused transform / team mode)");
    if (team_caller == 0 && e->p.Nc == 0) return fail(MATE_EINVAL, "the scenario has no cameras to act for");
    if (!c.action) return fail(MATE_EINVAL, "rollout_versus_greedy needs the %s team's joint action", team_caller == 0 ? "camera" : "target");
    if (team_caller >= 0 && (((g.act_discrete & 1) && team_caller == 0 && !g.cam_grid) || ((g.act_discrete & 2) && team_caller == 1 && !g.tgt_grid)))
        return fail(MATE_ESTATE, "discrete actions passed before mate_engine_set_action_grids");
    const LaunchPlan pl = plan_with_policies(e, per_step, team_caller);
    if (!pl.fits()) return fail(MATE_EINVAL, "rollout_greedy: %zu bytes of LDS per workgroup do not fit", pl.lds);
    g.mode = MODE_STEP; g.reset_kind = -1; g.rollout_steps = steps;
    g.parity = e->dev_tick ? 0 : e->parity;
    g.tick = e->dev_tick ? (uint32_t)e->steps_since_reset * (uint32_t)steps : e->tick;     // device-resident counter: the offset inside the reset interval
    g.tape_ct = nullptr; g.tape_goal = nullptr; g.freeze_done = 0;
    g.rotate_prio = e->sw.rollout_rotate;
    if (!flow.keep_list) g.done_count = nullptr;
    // pipelined restarts: this launch appends to list `parity`, which the reset launched two calls ago has consumed and cleared; the
    // environments that reset restarted carry this parity's tag and go live now
    if (pipelined && e->reset_in_flight[e->parity]) { HIP_TRY(hipStreamWaitEvent(stream, e->ev_reset[e->parity], 0)); e->reset_in_flight[e->parity] = false; }
    PolicyPtrs q = e->q;
    std::memset(&q.tape, 0, sizeof(q.tape));
    q.caller_team = team_caller;
    Timed t;
    MATE_TRY(take_timing_events(e, !e->dev_tick, &t));
    e->last_flow = pl.last_flow;
    e->opponents.consumed[MATE_TEAM_CAMERA] = e->opponents.consumed[MATE_TEAM_TARGET] = ROWS_GREEDY;      // (the joint actions of this launch are in q.cam_act / q.tgt_act: the Greedy agents', or the caller's)
    // (2d: the one-launch step holds its agents, so only the learner's routed messages mark; an engine-played team's trace needs its channel, which takes the two-launch
    // form.  This launch idles EVERY finished environment, whatever auto_reset is -- its record then says done = 2 --, so the trace's liveness rule is the record's done word alone)
    if (per_step) MATE_TRY(launch_trace(e, 1, stream));
    launch(pl.policy, dim3(pl.blocks), dim3(pl.threads), pl.lds, stream, t, e->d_params, g, q);
    HIP_TRY(hipGetLastError());
    e->selection.masks_stale = false;
    if (!e->dev_tick) e->tick += (uint32_t)steps;
    MATE_TRY(attached_behind_step(e, selected, io, steps, stream, per_step ? -1 : team_caller));
    return pipelined ? pipelined_restart(e, stream) : restart_finished(e, auto_reset, flow.restart, stream);
}

extern "C" int mate_engine_rollout_greedy(mate_engine *e, const mate_step_io *io, int32_t steps, int32_t auto_reset, void *stream) {
    return attached_last(e, rollout_with_policies(e, -1, io, steps, auto_reset, stream), (hipStream_t)stream);
}

extern "C" int mate_engine_rollout_versus_greedy(mate_engine *e, int32_t team, const mate_step_io *io, int32_t steps, int32_t auto_reset, void *stream) {
    if (team != MATE_TEAM_CAMERA && team != MATE_TEAM_TARGET) return fail(MATE_EINVAL, "team must be MATE_TEAM_CAMERA or MATE_TEAM_TARGET");
    return attached_last(e, rollout_with_policies(e, team, io, steps, auto_reset, stream), (hipStream_t)stream);
}

// Copy the joint actions the last mate_engine_step_greedy produced into caller buffers ([N][Nc][2], [N][Nt][2] f64): what that call's stepping launch
// read, and so until the NEXT stepping call -- a setter in between (opponent, mixture, channel) does not change what is reported.
extern "C" int mate_engine_policy_actions(mate_engine *e, double *camera_actions_dev, double *target_actions_dev, void *stream) {
    if (!e || !e->policy_ready) return fail(MATE_ESTATE, "policies are not enabled");
    HIP_TRY(hipSetDevice(e->device));
    note_stream(e, (hipStream_t)stream);
    double *const dst[2] = {e->p.Nc > 0 ? camera_actions_dev : nullptr, target_actions_dev};
    for (int team = 0; team < 2; ++team) {      // what the last call's step consumed (the caller's own rows are not the engine's to report: the Greedy buffer then, as ever)
        const double *src = rows_of(e, team, e->opponents.consumed[team]);
        if (dst[team]) HIP_TRY(hipMemcpyAsync(dst[team], src ? src : rows_of(e, team, ROWS_GREEDY), sizeof(double) * 2 * agents_of(e, team) * (size_t)e->N, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return MATE_OK;
}
extern "C" int mate_engine_policy_greedy_target_actions(mate_engine *e, double *target_actions_dev, void *stream) {
    if (!e || !e->policy_ready) return fail(MATE_ESTATE, "policies are not enabled");
    if (!target_actions_dev) return fail(MATE_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    note_stream(e, (hipStream_t)stream);
    HIP_TRY(hipMemcpyAsync(target_actions_dev, e->q.tgt_act, sizeof(double) * 2 * e->p.Nt * (size_t)e->N, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MATE_OK;
}

extern "C" int mate_engine_observe(mate_engine *e, const mate_step_io *io, void *stream) {
    return attached_last(e, launch_step(e, io, MODE_OBSERVE, 0, (hipStream_t)stream), (hipStream_t)stream);
}

extern "C" int mate_engine_export_state(mate_engine *e, double *dst_dev, void *stream) {
    if (!e || !dst_dev) return fail(MATE_EINVAL, "null argument");
    MATE_TRY(enter(e, (hipStream_t)stream));
    note_stream(e, (hipStream_t)stream);
    hipLaunchKernelGGL(export_kernel, dim3((unsigned)((e->N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, e->d_params, e->g, dst_dev);
    HIP_TRY(hipGetLastError());
    return MATE_OK;
}

extern "C" int mate_engine_import_state(mate_engine *e, const double *src_dev, void *stream) {
    if (!e || !src_dev) return fail(MATE_EINVAL, "null argument");
    if (e->dev_tick) return fail(MATE_ESTATE, "import_state while the step counter is device-resident (mate_engine_device_tick)");
    MATE_TRY(enter(e, (hipStream_t)stream));
    note_stream(e, (hipStream_t)stream);
    hipLaunchKernelGGL(import_kernel, dim3((unsigned)((e->N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, e->d_params, e->g, src_dev);
    HIP_TRY(hipGetLastError());
    MATE_TRY(clear_episode_sums(e, (hipStream_t)stream));
    MATE_TRY(clear_message_tags(e, (hipStream_t)stream));
    MATE_TRY(clear_trace_tags(e, (hipStream_t)stream));
    // all environments step together, so they share one tick: adopt the imported one
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    int32_t tick = 0;
    HIP_TRY(hipMemcpy(&tick, reinterpret_cast<const int32_t *>(e->g.dyn + e->p.DF) + e->p.Nt * TI_STRIDE + EI_TICK, sizeof(tick), hipMemcpyDeviceToHost));
    e->tick = (uint32_t)tick;
    e->was_reset = true; e->selection.masks_stale = true;      // (records only: the view masks are whatever ran before)
    return attached_behind_new_records(e, (hipStream_t)stream);
}

// One camera's knot table (inner or outer boundary) to the host / from the host.  `who`: the entry point's name in the messages.
static int lut_read_from(mate_engine *e, const double2 *knots_dev, const int32_t *counts_dev, int kmax, const char *who,
                         int64_t env, int32_t camera, double *phis, double *rhos, int32_t capacity, int32_t *count) {
    if (env < 0 || env >= e->N || camera < 0 || camera >= e->p.Nc) return fail(MATE_EINVAL, "%s: index out of range", who);
    MATE_TRY(enter_host(e));
    const int64_t lc = env * e->p.Nc + camera;
    int32_t n = 0;
    HIP_TRY(hipMemcpy(&n, counts_dev + lc, sizeof(n), hipMemcpyDeviceToHost));
    *count = n;
    if (n > capacity) return fail(MATE_EINVAL, "%s: capacity %d < %d knots", who, capacity, n);
    std::vector<double2> knots((size_t)n);
    HIP_TRY(hipMemcpy(knots.data(), knots_dev + lc * kmax, sizeof(double2) * (size_t)n, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) { phis[i] = knots[i].x; rhos[i] = knots[i].y; }
    return MATE_OK;
}
// (the front half of a write: the checks, the launches drained, the knots packed and on the device with their count)
static int lut_write_to(mate_engine *e, double2 *knots_dev, int32_t *counts_dev, int kmax, const char *who,
                        int64_t env, int32_t camera, const double *phis, const double *rhos, int32_t n) {
    if (env < 0 || env >= e->N || camera < 0 || camera >= e->p.Nc) return fail(MATE_EINVAL, "%s: index out of range", who);
    if (n < 2 || n > kmax) return fail(MATE_EINVAL, "%s: %d knots do not fit (capacity %d)", who, n, kmax);
    MATE_TRY(enter_host(e));
    std::vector<double2> knots((size_t)n);
    for (int i = 0; i < n; ++i) { knots[i].x = phis[i]; knots[i].y = rhos[i]; }
    const int64_t lc = env * e->p.Nc + camera;
    HIP_TRY(hipMemcpy(knots_dev + lc * kmax, knots.data(), sizeof(double2) * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(counts_dev + lc, &n, sizeof(n), hipMemcpyHostToDevice));
    return MATE_OK;
}

extern "C" int mate_engine_lut_read(mate_engine *e, int64_t env, int32_t camera, double *phis, double *rhos, int32_t capacity, int32_t *count) {
    if (!e || !phis || !rhos || !count) return fail(MATE_EINVAL, "null argument");
    return lut_read_from(e, e->g.lut_knots, e->g.lut_count, e->p.kmax, "lut_read", env, camera, phis, rhos, capacity, count);
}

extern "C" int mate_engine_lut_read_outer(mate_engine *e, int64_t env, int32_t camera, double *phis, double *rhos, int32_t capacity, int32_t *count) {
    if (!e || !phis || !rhos || !count) return fail(MATE_EINVAL, "null argument");
    if (!e->g.lut_knots_outer) return fail(MATE_ESTATE, "outer boundary not enabled (mate_engine_enable_outer_boundary)");
    return lut_read_from(e, e->g.lut_knots_outer, e->g.lut_count_outer, e->g.kmax_outer, "lut_read_outer", env, camera, phis, rhos, capacity, count);
}

// Camera.boundary_outer / sight_range_outer_func (entities.py:419-448, 479): built by every later reset /
// rebuild_luts next to the inner table.  Off by default: only boundary_between(outer=True) reads it.
extern "C" int mate_engine_enable_outer_boundary(mate_engine *e, int32_t *capacity) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    const Params &p = e->p;
    if (p.Nc == 0) return fail(MATE_EINVAL, "no cameras in this scenario");
    if (e->g.lut_knots_outer) { if (capacity) *capacity = e->g.kmax_outer; return MATE_OK; }
    MATE_TRY(enter_host(e));
    // 360 + per obstacle (arc <= 181 rays + two 21-point flanks) rays are sorted in LDS
    const int rays = 360 + p.No * (181 + 42) + 1;
    ResetLds rl = e->rl;
    layout_reset_lds(p, rl, std::max(rl.sort_cap, next_pow2(rays)));
    const int roff = rl.total_bytes;
    if (rl.sort_in_hbm && (!e->g.sort_scratch || rl.sort_cap != e->rl.sort_cap)) {      // the larger sort needs (larger) HBM scratch
        double *scratch = nullptr;
        int rc0 = dev_alloc(e, &scratch, (size_t)kSortGridCap * 4 * rl.sort_cap, false);
        if (rc0 != MATE_OK) return rc0;
        e->g.sort_scratch = scratch;
    }
    const int kmax_outer = round_up(rays + 2, 8);
    double2 *knots = nullptr; int32_t *counts = nullptr;
    int rc = dev_alloc(e, &knots, (size_t)e->N * p.Nc * kmax_outer);
    if (rc == MATE_OK) rc = dev_alloc(e, &counts, (size_t)e->N * p.Nc);
    if (rc != MATE_OK) return rc;
    const hipError_t err = with_obs_type(p.obs_f64 != 0, [&](auto tag) { return set_dynamic_lds(&reset_kernel<decltype(tag)>, (size_t)roff); });
    if (err != hipSuccess) return fail(MATE_EHIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(err));
    e->rl = rl; e->reset_lds = (size_t)roff;
    setup_two_tier(e);
    e->g.lut_knots_outer = knots; e->g.lut_count_outer = counts; e->g.kmax_outer = kmax_outer;
    if (capacity) *capacity = kmax_outer;
    return MATE_OK;
}

extern "C" int mate_engine_lut_write_outer(mate_engine *e, int64_t env, int32_t camera, const double *phis, const double *rhos, int32_t n) {
    if (!e || !phis || !rhos) return fail(MATE_EINVAL, "null argument");
    if (!e->g.lut_knots_outer) return fail(MATE_ESTATE, "outer boundary not enabled (mate_engine_enable_outer_boundary)");
    return lut_write_to(e, e->g.lut_knots_outer, e->g.lut_count_outer, e->g.kmax_outer, "lut_write_outer", env, camera, phis, rhos, n);
}

extern "C" int mate_engine_soft_coverage(mate_engine *e, const uint32_t *masks_dev, double *matrix_dev, double *scores_dev, void *stream) {
    if (!e || !masks_dev) return fail(MATE_EINVAL, "null argument");
    if (!matrix_dev && !scores_dev) return fail(MATE_EINVAL, "soft_coverage: no output buffer");
    if (e->p.Nc == 0) return fail(MATE_EINVAL, "no cameras in this scenario");
    if (e->p.Nt > kAuxMaxTargets) return fail(MATE_EINVAL, "soft_coverage: at most %d targets", kAuxMaxTargets);
    if (!e->g.lut_knots_outer) return fail(MATE_ESTATE, "outer boundary not enabled (mate_engine_enable_outer_boundary)");
    MATE_TRY(enter(e, (hipStream_t)stream, "soft_coverage"));
    note_stream(e, (hipStream_t)stream);
    launch_soft_coverage(e, plan_soft_coverage(e), masks_dev, matrix_dev, scores_dev, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MATE_OK;
}

extern "C" int mate_engine_lut_write(mate_engine *e, int64_t env, int32_t camera, const double *phis, const double *rhos, int32_t n) {
    if (!e || !phis || !rhos) return fail(MATE_EINVAL, "null argument");
    MATE_TRY(lut_write_to(e, e->g.lut_knots, e->g.lut_count, e->p.kmax, "lut_write", env, camera, phis, rhos, n));
    // the inner table's indices: built on the host, as the device builder in reset_kernels.hpp builds them
    std::vector<uint16_t> bucket((size_t)e->p.nbucket, 0);
    // per-degree index: bucket[d] = last knot with angle <= d - 180 (exact integer knots exist in real tables)
    int j = 0;
    for (int d = 0; d <= 361; ++d) {
        const double a = (double)(d > 360 ? 360 : d) - 180.0;
        while (j + 1 < n && phis[j + 1] <= a) ++j;
        bucket[d] = (uint16_t)j;
    }
    const int64_t lc = env * e->p.Nc + camera;
    // per-cell records (same rule as the device builder in reset_kernels.hpp: a cell's knots from the last one at or below its
    // start up to, not including, the first one at or above the next cell's start)
    std::vector<double2> deg((size_t)kLutCells * kDegWords);
    const double inf = INFINITY;
    for (int cell = 0; cell < kLutCells; ++cell) {
        const int d = cell / kCellsPerDegree, sub = cell - d * kCellsPerDegree;
        int start = bucket[d];                                   // last knot with angle <= d - 180
        if (sub > 0) { const double a = cell_start(cell); while (start + 1 < n && phis[start + 1] <= a) ++start; }
        int endk = bucket[d + 1];
        if (sub < kCellsPerDegree - 1) { const double a = cell_start(cell + 1); endk = start; while (endk + 1 < n && phis[endk] < a) ++endk; }
        double2 *rec = deg.data() + (size_t)cell * kDegWords;
        double *words = reinterpret_cast<double *>(rec);
        // a caller's table may repeat an angle (np.interp repairs the infinite slope): such a cell takes the general path; so does
        // one whose degree does not start on a knot (real tables have a knot on every integer degree, and the closing knot of a
        // degree's last cell is taken from there)
        bool increasing = endk > start;
        for (int idx = start; idx < endk; ++idx) increasing = increasing && phis[idx + 1] > phis[idx];
        increasing = increasing && phis[bucket[d]] == (double)(d - 180) && phis[start] <= cell_start(cell) && phis[endk] >= cell_start(cell + 1);
        if (endk - start + 1 <= kDegSlots && increasing) {
            for (int i = 0; i < kDegSlots - 1; ++i) {
                const int idx = start + i;
                words[3 * i] = idx < endk ? phis[idx] : inf;
                words[3 * i + 1] = idx < endk ? rhos[idx] : 0.0;
                words[3 * i + 2] = idx < endk ? (rhos[idx + 1] - rhos[idx]) / (phis[idx + 1] - phis[idx]) : 0.0;
            }
        } else {
            for (int i = 0; i < kDegWords; ++i) { rec[i].x = NAN; rec[i].y = 0.0; }
            if (increasing) {                                                  // burst path: first knot, count, pivot stride, eight pivots
                const int count = endk - start + 1, last = count - 1;
                const int q = count <= kPivotKnots ? pivot_stride(count) : 0;
                rec[0].y = (double)start; rec[1].x = (double)count; rec[1].y = (double)q;
                for (int i = 0; i < 4; ++i) {
                    const int ka = (2 * i + 1) * q, kb = (2 * i + 2) * q;
                    rec[2 + i].x = q > 0 && ka <= last ? phis[start + ka] : inf;
                    rec[2 + i].y = q > 0 && kb <= last ? phis[start + kb] : inf;
                }
            }
            else rec[1].x = 0.0;                                                                                   // general path
        }
    }
    HIP_TRY(hipMemcpy(e->g.lut_deg + lc * kLutCells * kDegWords, deg.data(), sizeof(double2) * deg.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->g.lut_bucket + lc * e->p.nbucket, bucket.data(), sizeof(uint16_t) * bucket.size(), hipMemcpyHostToDevice));
    return MATE_OK;
}

// Debug hook (not part of the stable ABI): per-environment s_memtime stamps at the phase boundaries of
// the step kernel; only filled by builds with -DMATE_PHASE_CLOCKS.
extern "C" int mate_engine_debug_phase_clocks(mate_engine *e, long long *buf_dev) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    e->g.phase_clocks = buf_dev;
    return MATE_OK;
}
extern "C" int mate_engine_debug_skip(mate_engine *e, int32_t mask) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    e->g.debug_skip = mask;
    return MATE_OK;
}

// Total number of (environment, step) slots spent idle waiting for a batched reset (auto_reset > 1) since creation.
extern "C" int mate_engine_idle_steps(mate_engine *e, int64_t *total) {
    if (!e || !total) return fail(MATE_EINVAL, "null argument");
    MATE_TRY(enter_host(e));
    std::vector<int32_t> host((size_t)e->N);
    HIP_TRY(hipMemcpy(host.data(), e->g.idle_steps, sizeof(int32_t) * host.size(), hipMemcpyDeviceToHost));
    int64_t sum = 0;
    for (int32_t v : host) sum += v;
    *total = sum;
    return MATE_OK;
}

extern "C" int mate_engine_last_flow(const mate_engine *e) { return e ? e->last_flow : MATE_EINVAL; }

extern "C" int mate_engine_set_store_form(mate_engine *e, int32_t shifted) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    e->g.store_shifted = shifted ? 1 : 0;
    return MATE_OK;
}

// ---- observation blocks from shuffled 2 MiB physical chunks (include/mate_engine.h: mate_engine_block_alloc)
namespace {
struct ScatteredBlock { int device; size_t bytes; std::vector<hipMemGenericAllocationHandle_t> chunks; };
std::mutex g_blocks_mutex;
std::map<void *, ScatteredBlock> g_blocks;
std::atomic<int64_t> g_dead_range_bytes{0};      // address ranges of freed blocks that stay reserved (block_free)
constexpr size_t kBlockChunk = (size_t)2 << 20;      // smaller chunks cost TLB reach (1 MiB: 4.1-4.7 TB/s), larger ones scatter less
}  // namespace

extern "C" int mate_engine_block_alloc(int32_t device, int64_t bytes, void **ptr_out) {
    if (!ptr_out || bytes <= 0) return fail(MATE_EINVAL, "block_alloc: null output or empty block");
    *ptr_out = nullptr;
    HIP_TRY(hipSetDevice(device));
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = device;
    size_t granularity = 0;
    HIP_TRY(hipMemGetAllocationGranularity(&granularity, &prop, hipMemAllocationGranularityMinimum));
    if (granularity == 0 || kBlockChunk % granularity != 0) return fail(MATE_EHIP, "block_alloc: allocation granularity %zu does not divide 2 MiB", granularity);
    const size_t n = ((size_t)bytes + kBlockChunk - 1) / kBlockChunk, total = n * kBlockChunk;
    {   // refuse at once what the device cannot hold (creating chunk after chunk until the driver says no takes minutes for a terabyte)
        size_t free_bytes = 0, total_bytes = 0;
        HIP_TRY(hipMemGetInfo(&free_bytes, &total_bytes));
        if (total > free_bytes) return fail(MATE_ENOMEM, "block_alloc: %zu bytes asked for, %zu free on device %d", total, free_bytes, device);
    }
    // Address ranges of freed blocks stay reserved (block_free): refuse new blocks once a process has retired more than
    // MATE_BLOCK_DEAD_GIB (default 4096 GiB of the 2^47-byte address space) -- a loop that reallocates rollout buffers forever
    // gets an error it can read (the Python host then falls back to plain memory), not an address space that runs dry.
    static const int64_t dead_cap = [] { const char *v = getenv("MATE_BLOCK_DEAD_GIB"); return (int64_t)(v ? atof(v) : 4096.0) << 30; }();
    if (g_dead_range_bytes.load() + (int64_t)total > dead_cap && g_dead_range_bytes.load() > 0)
        return fail(MATE_ENOMEM, "block_alloc: %lld GiB of address space are held by freed blocks (limit MATE_BLOCK_DEAD_GIB = %lld): use plain device memory",
                    (long long)(g_dead_range_bytes.load() >> 30), (long long)(dead_cap >> 30));
    void *va = nullptr;
    HIP_TRY(hipMemAddressReserve(&va, total, kBlockChunk, nullptr, 0));
    ScatteredBlock blk{device, total, {}};
    blk.chunks.reserve(n);
    auto undo = [&](size_t mapped) {
        for (size_t i = 0; i < mapped; ++i) (void)hipMemUnmap((char *)va + i * kBlockChunk, kBlockChunk);
        for (auto h : blk.chunks) (void)hipMemRelease(h);
        (void)hipMemAddressFree(va, total);
        (void)hipGetLastError();      // (the sticky error of the call that failed: reported through the return code, not through the next launch check)
    };
    for (size_t i = 0; i < n; ++i) {
        hipMemGenericAllocationHandle_t h;
        const hipError_t err = hipMemCreate(&h, kBlockChunk, &prop, 0);
        if (err != hipSuccess) { undo(0); return fail(MATE_EHIP, "block_alloc: hipMemCreate failed after %zu of %zu chunks: %s", i, n, hipGetErrorString(err)); }
        blk.chunks.push_back(h);
    }
    // the chunks come out of the driver in address order, more or less: slot i of the virtual range takes chunk order[i]
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = i;
    std::mt19937_64 rng(0x9e3779b97f4a7c15ull ^ (uint64_t)(uintptr_t)va);
    std::shuffle(order.begin(), order.end(), rng);
    for (size_t i = 0; i < n; ++i) {
        const hipError_t err = hipMemMap((char *)va + i * kBlockChunk, kBlockChunk, 0, blk.chunks[order[i]], 0);
        if (err != hipSuccess) { undo(i); return fail(MATE_EHIP, "block_alloc: hipMemMap failed: %s", hipGetErrorString(err)); }
    }
    hipMemAccessDesc access = {};
    access.location = prop.location;
    access.flags = hipMemAccessFlagsProtReadWrite;
    {
        const hipError_t err = hipMemSetAccess(va, total, &access, 1);
        if (err != hipSuccess) { undo(n); return fail(MATE_EHIP, "block_alloc: hipMemSetAccess failed: %s", hipGetErrorString(err)); }
    }
    std::lock_guard<std::mutex> lock(g_blocks_mutex);
    g_blocks.emplace(va, std::move(blk));
    *ptr_out = va;
    return MATE_OK;
}

namespace {
// the store pattern of image_store / pack_rows_f32 on one block: row r * rows_per_step + env, by the wave that owns env
__global__ __launch_bounds__(256, 4) void block_probe_kernel(char *block, int64_t steps, int32_t rows_per_step, int32_t row_chunks) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t env = (int64_t)blockIdx.x * 4 + wave;
    if (env >= rows_per_step) return;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int64_t r = 0; r < steps; ++r) {
        f32x4 *row = reinterpret_cast<f32x4 *>(block) + (r * rows_per_step + env) * row_chunks;
        for (int s = lane; s < row_chunks; s += 64) __builtin_nontemporal_store(zero, row + s);
    }
}
}  // namespace

extern "C" int mate_engine_block_probe(int32_t device, void *block, int64_t bytes, int32_t rows_per_step, int32_t row_bytes, void *stream,
                                       double *gbytes_per_s) {
    if (!block || !gbytes_per_s || rows_per_step <= 0 || row_bytes <= 0 || row_bytes % 16 != 0) return fail(MATE_EINVAL, "block_probe: null block / rate or a row that is no multiple of 16 bytes");
    const int64_t steps = bytes / ((int64_t)rows_per_step * row_bytes);
    if (steps <= 0) return fail(MATE_EINVAL, "block_probe: the block holds less than one step of rows");
    HIP_TRY(hipSetDevice(device));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float best = 0.f;
    auto measure = [&]() -> hipError_t {
        hipError_t err;
        if ((err = hipEventCreate(&e0)) != hipSuccess) return err;
        if ((err = hipEventCreate(&e1)) != hipSuccess) return err;
        for (int rep = 0; rep < 4; ++rep) {      // (the first launch also pages the kernel in)
            if ((err = hipEventRecord(e0, (hipStream_t)stream)) != hipSuccess) return err;
            hipLaunchKernelGGL(block_probe_kernel, dim3((unsigned)((rows_per_step + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (char *)block, steps, rows_per_step, row_bytes / 16);
            if ((err = hipGetLastError()) != hipSuccess) return err;
            if ((err = hipEventRecord(e1, (hipStream_t)stream)) != hipSuccess) return err;
            if ((err = hipEventSynchronize(e1)) != hipSuccess) return err;
            float ms = 0.f;
            if ((err = hipEventElapsedTime(&ms, e0, e1)) != hipSuccess) return err;
            if (rep > 0 && (best == 0.f || ms < best)) best = ms;
        }
        return hipSuccess;
    };
    const hipError_t probe_err = measure();
    if (e0) (void)hipEventDestroy(e0);       // (on the error paths too)
    if (e1) (void)hipEventDestroy(e1);
    if (probe_err != hipSuccess) { (void)hipGetLastError(); return fail(MATE_EHIP, "block_probe: %s", hipGetErrorString(probe_err)); }
    const int64_t tail = bytes - steps * rows_per_step * row_bytes;
    if (tail > 0) HIP_TRY(hipMemsetAsync((char *)block + (bytes - tail), 0, (size_t)tail, (hipStream_t)stream));
    *gbytes_per_s = (double)(steps * rows_per_step) * row_bytes / ((double)best * 1e6);
    return MATE_OK;
}

namespace {
// the three rates a streaming kernel of this library can be priced against on THIS GPU: 16 bytes per lane, grid-stride, the
// non-temporal stores the row writers use.  mode 0: read src + write dst; 1: write dst only; 2: read src only (folded into one word
// per lane that is stored only if it equals a value it cannot have)
__global__ __launch_bounds__(256) void hbm_probe_kernel(const char *src, char *dst, int64_t chunks, int32_t mode) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const f32x4 *in = reinterpret_cast<const f32x4 *>(src);
    f32x4 *out = reinterpret_cast<f32x4 *>(dst);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const f32x4 fill = {1.f, 2.f, 3.f, 4.f};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < chunks; i += stride) {
        if (mode == 0) __builtin_nontemporal_store(__builtin_nontemporal_load(in + i), out + i);
        else if (mode == 1) __builtin_nontemporal_store(fill, out + i);
        else if (mode == 3) out[i] = fill;                       // (plain stores: what a memset does)
        else acc += __builtin_nontemporal_load(in + i);
    }
    if (mode == 2 && acc.x + acc.y + acc.z + acc.w == -1.2345e30f) out[0] = acc;
}
}  // namespace

extern "C" int mate_engine_hbm_probe(int32_t device, const void *src, void *dst, int64_t bytes, int32_t mode, void *stream, double *gbytes_per_s) {
    if (!gbytes_per_s || bytes < 16 || mode < 0 || mode > 3 || !dst || ((mode == 0 || mode == 2) && !src))
        return fail(MATE_EINVAL, "hbm_probe: null rate / buffer, fewer than 16 bytes or a mode other than 0 (copy), 1 (fill, non-temporal), 2 (read), 3 (fill, plain stores)");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    const int64_t chunks = bytes / 16;
    // (a copy / read runs best with a few resident workgroups per CU striding over the buffer; a fill with one thread per few chunks)
    const unsigned grid = (unsigned)std::min<int64_t>((chunks + 255) / 256, (int64_t)prop.multiProcessorCount * ((mode == 1 || mode == 3) ? 64 : 8));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::vector<float> ms_all;
    auto measure = [&]() -> hipError_t {
        hipError_t err;
        if ((err = hipEventCreate(&e0)) != hipSuccess) return err;
        if ((err = hipEventCreate(&e1)) != hipSuccess) return err;
        for (int rep = 0; rep < 6; ++rep) {      // (the first launch also pages the kernel in)
            if ((err = hipEventRecord(e0, (hipStream_t)stream)) != hipSuccess) return err;
            hipLaunchKernelGGL(hbm_probe_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const char *)src, (char *)dst, chunks, mode);
            if ((err = hipGetLastError()) != hipSuccess) return err;
            if ((err = hipEventRecord(e1, (hipStream_t)stream)) != hipSuccess) return err;
            if ((err = hipEventSynchronize(e1)) != hipSuccess) return err;
            float ms = 0.f;
            if ((err = hipEventElapsedTime(&ms, e0, e1)) != hipSuccess) return err;
            if (rep > 0) ms_all.push_back(ms);
        }
        return hipSuccess;
    };
    const hipError_t probe_err = measure();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (probe_err != hipSuccess) { (void)hipGetLastError(); return fail(MATE_EHIP, "hbm_probe: %s", hipGetErrorString(probe_err)); }
    std::sort(ms_all.begin(), ms_all.end());
    const double ms = ms_all[ms_all.size() / 2];          // the median of five
    *gbytes_per_s = (double)(chunks * 16) * (mode == 0 ? 2.0 : 1.0) / (ms * 1e6);
    return MATE_OK;
}

extern "C" int mate_engine_set_sub_wave(mate_engine *e, int32_t enable, int32_t *in_use) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    if (enable > 2) return fail(MATE_EINVAL, "set_sub_wave: 0 (one per wave), 1 (the shape's number), 2 (where it measured faster) or negative (query)");
    if (enable >= 0) e->sw.sub_wave_mode = enable;      // (negative: a query)
    if (in_use) { in_use[0] = plan_with_policies(e, false, -1).E; }
    return MATE_OK;
}

extern "C" int mate_engine_memory_hold(int32_t device, int64_t bytes, void **token_out) {
    if (!token_out || bytes <= 0) return fail(MATE_EINVAL, "memory_hold: null output or nothing to hold");
    *token_out = nullptr;
    HIP_TRY(hipSetDevice(device));
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = device;
    constexpr size_t piece = (size_t)256 << 20;
    auto *held = new std::vector<hipMemGenericAllocationHandle_t>();
    for (size_t done = 0; done < (size_t)bytes; done += piece) {
        hipMemGenericAllocationHandle_t h;
        const hipError_t err = hipMemCreate(&h, piece, &prop, 0);
        if (err != hipSuccess) {
            for (auto x : *held) (void)hipMemRelease(x);
            delete held;
            (void)hipGetLastError();
            return fail(MATE_ENOMEM, "memory_hold: hipMemCreate failed after %zu bytes: %s", done, hipGetErrorString(err));
        }
        held->push_back(h);
    }
    *token_out = held;
    return MATE_OK;
}

extern "C" int mate_engine_memory_release(void *token) {
    if (!token) return MATE_OK;
    auto *held = static_cast<std::vector<hipMemGenericAllocationHandle_t> *>(token);
    for (auto h : *held) (void)hipMemRelease(h);
    delete held;
    return MATE_OK;
}

extern "C" int mate_engine_block_free(void *ptr) {
    if (!ptr) return MATE_OK;
    ScatteredBlock blk;
    {
        std::lock_guard<std::mutex> lock(g_blocks_mutex);
        auto it = g_blocks.find(ptr);
        if (it == g_blocks.end()) return fail(MATE_EINVAL, "block_free: %p was not returned by mate_engine_block_alloc", ptr);
        blk = std::move(it->second);
        g_blocks.erase(it);
    }
    hipError_t first = hipSetDevice(blk.device);
    // One hipMemUnmap per hipMemMap: the runtime keeps a record per mapping, and a single unmap of the whole range (rounds 1-3)
    // retired only the first chunk's -- the other chunks stayed mapped behind a range the next reservation could receive,
    // which is how "a reused range lost rows of the next rollout" came about.  Every step runs even after a failure (the
    // remaining chunks are still worth releasing); the first error is reported.
    const size_t n = blk.chunks.size();
    for (size_t i = 0; i < n; ++i) {
        const hipError_t err = hipMemUnmap((char *)ptr + i * kBlockChunk, kBlockChunk);
        if (err != hipSuccess && first == hipSuccess) first = err;
    }
    for (auto h : blk.chunks) {
        const hipError_t err = hipMemRelease(h);
        if (err != hipSuccess && first == hipSuccess) first = err;
    }
    // The virtual range stays reserved for the life of the process (address space only: 2^47 bytes of it, a block is a few GB)
    // unless MATE_BLOCK_FREE_RANGE=1: with every chunk properly unmapped a range handed out AGAIN still lost rows of the next
    // rollout in two of four runs of the GPU suite (tools/va_reuse.hip is the minimal repro).
    static const bool free_range = [] { const char *v = getenv("MATE_BLOCK_FREE_RANGE"); return v && atoi(v) != 0; }();
    if (free_range) {
        const hipError_t err = hipMemAddressFree(ptr, blk.bytes);
        if (err != hipSuccess && first == hipSuccess) first = err;
    } else g_dead_range_bytes += (int64_t)blk.bytes;      // (bounded: block_alloc refuses beyond MATE_BLOCK_DEAD_GIB)
    if (first != hipSuccess) {
        (void)hipGetLastError();
        return fail(MATE_EHIP, "block_free: %s", hipGetErrorString(first));
    }
    return MATE_OK;
}

extern "C" int mate_engine_kernel_time(mate_engine *e, int32_t enable, double *avg_ms, int64_t *launches) {
    if (!e) return fail(MATE_EINVAL, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    double total = 0.0;
    int64_t n = 0;
    if (e->events_used) {
        HIP_TRY(wait_for_launches(e));
        for (size_t i = 0; i < e->events_used; ++i) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, e->events[i].first, e->events[i].second));
            total += ms; ++n;
        }
    }
    if (avg_ms) *avg_ms = n ? total / (double)n : 0.0;
    if (launches) *launches = n;
    e->events_used = 0;
    e->timing = enable > 0 ? enable : 0;
    e->timing_tick = 0;
    return MATE_OK;
}
