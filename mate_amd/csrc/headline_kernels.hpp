// headline_kernels.hpp -- the fused random-policy rollout of ONE form, the headline's: MATE-4v8-9 (FixedShape 4 / 8 / 9), row image, held lane roles,
// held step state, f32 rows, one environment per wave.  It is rollout_kernel<float, FixedShape<4, 8, 9, false, true>, FLOW_RANDOM, 1> (engine_kernels.hpp)
// with the branches of the other forms folded away, its own versions of what moves the rows, and the cameras' kinematics -- the one phase that needs
// nothing of the step it runs in -- computed sixteen steps per pass (headline_camera_pass, headline_camera_step) with the shared math, bit for bit:
//   * headline_blocks   a pair's verdict selects the SOURCE of its block (the other's public state, or a block of zeros) instead of masking the
//                       four to seven words that were read: same bytes (x & ~0 = x, x & 0 = the zero word), one select per pair;
//   * headline_store    the row store: its form (Ptrs::store_shifted) is a template parameter of the kernel -- one form per instantiation, no branch per
//                       step -- and the rows' global addresses are running 64-bit scalars advanced by N rows per step, not row index times row size.
// The loop head is rollout_kernel's: with the launch arguments read once ahead of the loop (passed by value instead of through kernarg_ptrs) the compiler
// spills 42 scalar registers instead of 13 and reloads them with 75 v_readlane per step instead of 21 -- on the unit that bounds the kernel -- so they are
// still read where they are used.
// Every other phase that computes (draws, the targets' kinematics, views, scores) and the prologue / epilogue are the shared functions, called as
// rollout_kernel calls them.
// The kernels live in a translation unit of their own (headline_kernels.hip) with a resource report of their own (mate_amd/build.py:
// lib/kernel_resources_headline.json); the host picks them per launch (engine_host.h: plan_rollout_random).  No profiling stamps, no phase ablation,
// no debug_skip: a launch that asks for any of them runs rollout_kernel.
#pragma once
#include "engine_kernels.hpp"

namespace mate {

using HeadlineShape = FixedShape<4, 8, 9, false, true>;
constexpr int kHeadlineZeroBytes = 32;      // the zero block behind the workgroup's four slices: a camera's block reads 16 + 12 bytes of it
// dynamic LDS of a workgroup: four environments' slices and the zero block
constexpr size_t headline_lds_bytes(size_t image_wave_bytes) { return 4 * image_wave_bytes + kHeadlineZeroBytes; }

#if defined(MATE_ISA_MARKS)
#define HEADLINE_MARK(i) asm volatile("; ==== MATE_PHASE_END " #i)      // (tools/isa_phases.py cuts the kernel's text at these)
#else
#define HEADLINE_MARK(i) do { } while (0)
#endif

// image_blocks with the verdict on the address: `zero` is the LDS address of kHeadlineZeroBytes zero bytes.  As there, every lane reads in every slot (one
// without a block reads offset 0 of its slice, or the zero block: harmless) and every read is issued before the first write.
// (Measured on the compiler: reads under the lanes' own conditions -- as wide as the block, none without one -- come back as copies of every word
// into the registers the writes expect, 120 moves per step and 56 spilled registers.)
template <int ROUNDS>
__device__ __forceinline__ void headline_blocks(Ctx<float> &c, const RangeRoles &roles, uint32_t seen, uint32_t zero) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) const u32x4 lds_cu4;
    const uint32_t slice = lds_addr(c.base);
    u32x4 a[1 + ROUNDS], b[1 + ROUNDS];
#pragma unroll
    for (int slot = 0; slot < 1 + ROUNDS; ++slot) {
        const uint32_t src = ((seen >> slot) & 1u) ? slice + (roles.block[slot] & 0xffffu) : zero;
        a[slot] = *(lds_cu4 *)(uintptr_t)src; b[slot] = *(lds_cu4 *)(uintptr_t)(src + 16u);
    }
    // (every slot's reads in flight before the first write: left alone, the compiler sinks a slot's reads into the branch that writes its block -- a second round trip)
#pragma unroll
    for (int slot = 0; slot < 1 + ROUNDS; ++slot) asm volatile("" : "+v"(a[slot]), "+v"(b[slot]));
#pragma unroll
    for (int slot = 0; slot < 1 + ROUNDS; ++slot) {
        const uint32_t code = (roles.block_bits >> (2 * slot)) & 3u;
        if (code != 0u) {
            uint32_t *dst = reinterpret_cast<uint32_t *>(c.base + (roles.block[slot] >> 16));
            dst[0] = a[slot].x; dst[1] = a[slot].y; dst[2] = a[slot].z; dst[3] = a[slot].w;
            if (code >= 2u) dst[4] = b[slot].x;
            if (code == 3u) { dst[5] = b[slot].y; dst[6] = b[slot].z; }
        }
    }
    wave_sync();
}

// image_store_form for this shape (128 camera chunks, 260 target chunks of 16 bytes) over RUNNING row addresses: `row_c` / `row_t` are the global addresses of
// this environment's camera / target block in the step's row, held in scalar registers and advanced by the launch's stride (N rows) behind every step --
// no row index times row size per step, and the shift of the line-aligned form is bits 4-6 of the address itself.  As there: all LDS reads of a block
// before its first store.  (The addresses are in registers since the prologue: no pointer's round trip stands in front of the reads.)
template <bool SHIFTED>
__device__ __forceinline__ void headline_store(const Ctx<float> &c, uint64_t row_c, uint64_t row_t) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(1))) f32x4 global_f32x4;
    constexpr int nvc = HeadlineShape::kChunksC, nvt = HeadlineShape::kChunksT;
    constexpr int slack = SHIFTED ? 7 : 0;
    constexpr int GC = (nvc + slack + 63) / 64, GT = (nvt + slack + 63) / 64;
    static_assert(GC <= 3 && GT <= 7, "image_fits: at most 3 + 7 rounds");
    const int lane = c.lane & 63;
    const int sc = SHIFTED ? (int)((uint32_t)(row_c >> 4) & 7u) : 0, st = SHIFTED ? (int)((uint32_t)(row_t >> 4) & 7u) : 0;
    const f32x4 *from_c = reinterpret_cast<const f32x4 *>(c.img) - sc, *from_t = reinterpret_cast<const f32x4 *>(c.img + 4 * nvc) - st;
    f32x4 vc[GC], vt[GT];
#pragma unroll
    for (int k = 0; k < GC; ++k) vc[k] = from_c[lane + 64 * k];
#pragma unroll
    for (int k = 0; k < GT; ++k) vt[k] = from_t[lane + 64 * k];
    global_f32x4 *to_c = (global_f32x4 *)row_c - sc, *to_t = (global_f32x4 *)row_t - st;
#pragma unroll
    for (int k = 0; k < GC; ++k) {
        const bool inside = (k > 0 || lane >= sc) && (64 * (k + 1) <= nvc || lane + 64 * k - sc < nvc);
        if (inside) stream_store(vc[k], &to_c[lane + 64 * k]);
    }
#pragma unroll
    for (int k = 0; k < GT; ++k) {
        const bool inside = (k > 0 || lane >= st) && (64 * (k + 1) <= nvt || lane + 64 * k - st < nvt);
        if (inside) stream_store(vt[k], &to_t[lane + 64 * k]);
    }
}

// The cameras, sixteen steps per pass.  Under the random policy a camera's kinematics (simulate_cameras_held) are a function of its previous (ph, th) and
// its own Philox words alone -- targets, views, goals and the episode's bookkeeping never feed back into them -- and run on 4 of 64 lanes at every step.
// Here lane l stands for camera l >> 4 at step tick + (l & 15): one 64-lane Philox call, a scan of (ph, th) down each row of sixteen lanes, the pointwise
// part (quotient, sine / cosine, root, products) once on every lane, and the lane keeps its step's values until headline_camera_step hands them over.
// Same operations in the same order as step_draws and simulate_cameras_held: same bits.
struct CameraAhead { double ph, th, sr2; float x, y; };

// a row's lane takes `v` of the lane below it (DPP row_shr:1); the row's first lane keeps `keep`
__device__ __forceinline__ double headline_row_pred(double keep, double v) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(keep), __double2loint(v), 0x111, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(keep), __double2hiint(v), 0x111, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// `tick`: the tick of the step at hand (the row's first lane's).  The cameras' current pair is the record's in LDS, c.phi / c.theta: written at every step,
// and what a launch, a restart or an imported state starts from.
__device__ __forceinline__ void headline_camera_pass(Ctx<float> &c, uint32_t tick, CameraAhead &a) {
    const Params &p = c.p;
    const int cam = c.lane >> 4;
    const uint32_t t = tick + (uint32_t)(c.lane & 15);
    // the lane's own block; the two lanes that share one compute it twice (no carry, no parity case)
    const U4 w = philox(p.seed_lo, p.seed_hi, c.env_global(), t >> 1, S_ACT_CAM, (uint32_t)cam);
    const uint32_t w0 = (t & 1u) ? w.z : w.x, w1 = (t & 1u) ? w.w : w.y;
    const double da = clip_uniform(action_component(w0, p.rot), -p.rot, p.rot);
    const double dz = clip_uniform(action_component(w1, p.zoom), -p.zoom, p.zoom);
    // the scan, systolic: in round j every lane steps from the pair of the lane below it, the row's first lane from the camera's current pair; behind
    // round j the lanes 0..j of a row hold their step's pair (a lane above them holds a pair stepped from an unfinished one: an angle in range like any other)
    double pph = c.phi(cam), pth = c.theta(cam);
    double ph = normalize_angle(pph + da);
    double th = clip_uniform(pth + dz, p.theta_min, kMaxViewingAngle);
#pragma clang loop unroll(disable)
    for (int j = 1; j < 16; ++j) {
        pph = headline_row_pred(pph, ph); pth = headline_row_pred(pth, th);
        ph = normalize_angle(pph + da);
        th = clip_uniform(pth + dz, p.theta_min, kMaxViewingAngle);
    }
    const double sr2 = div_nz(p.area, th);
    float sn, cs;
    sincos_deg_f32(ph, sn, cs);
    const float srf = sqrt_f32_1ulp((float)sr2);
    a.ph = ph; a.th = th; a.sr2 = sr2; a.x = srf * cs; a.y = srf * sn;
}

// The step's hand-over, in place of simulate_cameras_held: the four lanes whose step this is write the words it writes.
__device__ __forceinline__ void headline_camera_step(Ctx<float> &c, int r, const CameraAhead &a) {
    if ((c.lane & 15) == (r & 15)) {
        const int cam = c.lane >> 4;
        c.phi(cam) = a.ph; c.theta(cam) = a.th;                // (the sector tests of the pair lanes read these)
        c.sight2(cam) = a.sr2;
        float *pc = c.pub_cam(cam), *row = c.img_cam_row(cam) + 13;
        const float tf = (float)a.th;
        pc[3] = a.x; pc[4] = a.y; pc[5] = tf; row[3] = a.x; row[4] = a.y; row[5] = tf;
    }
}

// `SHIFTED`: the form of the row stores (image_store_form), what Ptrs::store_shifted says for this launch -- the host launches the instantiation that matches.
template <bool SHIFTED>
__global__ __launch_bounds__(256, 4) void headline_rollout_kernel(const Params *__restrict__ pp, const Ptrs g) {
    using Shape = HeadlineShape;
    constexpr int FLOW = FLOW_RANDOM;
    static_assert(Shape::kImage && Shape::kHoldRoles && shape_range_rounds(4, 8, 9) == 3, "the headline form: row image, held roles, three range rounds");
    const Shape shape(pp, true);
    const Params &p = shape.get();
    extern __shared__ __align__(16) unsigned char smem[];
    if (blockIdx.x == 0 && threadIdx.x == 0 && g.done_count) g.done_count[g.parity ^ 1] = 0;
    // wave-uniform by construction; readfirstlane lets the compiler keep everything derived from it in SGPRs
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int64_t env = (int64_t)blockIdx.x * 4 + wave;
    if (env >= g.N) return;
    const Ptrs &gk = kernarg_ptrs(g);     // launch arguments read where they are used (see step_kernel)
    // the zero block, by every wave of the workgroup for itself (the same bytes: no wave waits for another); visible behind the prologue's first wave_sync
    unsigned char *const zero_block = smem + 4 * p.lds_wave_bytes;
    if (lane < kHeadlineZeroBytes / 4) reinterpret_cast<uint32_t *>(zero_block)[lane] = 0u;
    const uint32_t zero = lds_addr(zero_block);
    {
        Ctx<float> c(p, gk, smem + wave * p.lds_wave_bytes, lane, env, FLOW_ANY);
        load_records(c);
        wave_sync();
        build_entities(c);
        list_finished_at_entry(c);
        wave_sync();
    }
    RangeRoles roles;                        // the lane's range-test pairs and limits, static inside an episode
    {
        Ctx<float> c(p, gk, smem + wave * p.lds_wave_bytes, lane, env, FLOW);
        range_roles(c, roles);
        pin_roles(roles);
        image_statics(c);
    }
    NearCarry near{};                       // the collision screen of the step to come, made by the range tests of the step before
    {
        Ctx<float> c(p, gk, smem + wave * p.lds_wave_bytes, lane, env, FLOW);
        near_seed(c, roles, near);
    }
    // fair shares of the SIMD: the issue priority rotates by step and wave slot (rollout_kernel says why)
    uint32_t hw_id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
    const int wave_slot = (int)(hw_id & 15u);
    bool stepped = false;            // a full step has written the static mask words
    int last_gw = -1;                // the goal word behind the target's goal / cargo slots
    DrawCarry carry{0u, 0u, 0xffffffffu};
    DrawRole draws_of_lane;
    {
        Ctx<float> c(p, gk, smem + wave * p.lds_wave_bytes, lane, env, FLOW);
        draws_of_lane = draw_role(c);
    }
    HeldState h{};
    CameraAhead ahead{};             // the lane's camera step of the pass at hand (headline_camera_pass)
    int finished = 0;                // the episode is over (wave-uniform)
    const uint32_t tick0 = g.tick;   // (launch arguments read once: inside the loop each read is a scalar load and a wait)
    const int n_steps = g.rollout_steps;
    // this environment's blocks in the row of the step at hand, and what a step adds: N rows
    constexpr uint64_t kRowC = (uint64_t)Shape::kChunksC * 16u, kRowT = (uint64_t)Shape::kChunksT * 16u;
    uint64_t row_c = reinterpret_cast<uint64_t>(g.cam_obs) + (uint64_t)env * kRowC, row_t = reinterpret_cast<uint64_t>(g.tgt_obs) + (uint64_t)env * kRowT;
    const uint64_t step_c = (uint64_t)g.N * kRowC, step_t = (uint64_t)g.N * kRowT;
    {
        Ctx<float> c(p, gk, smem + wave * p.lds_wave_bytes, lane, env, FLOW);
        held_load(c, h);
        finished = __builtin_amdgcn_readfirstlane((int)(c.ei(EI_DONE) != 0));
    }
#pragma clang loop unroll(disable)
    for (int r = 0; r < n_steps; ++r, row_c += step_c, row_t += step_t) {
        // an opaque copy of the lane id per iteration keeps the compiler from hoisting every lane-role
        // computation of the body out of the loop (which costs >100 VGPRs of spills)
        int lane_r = lane, wave_r = wave;
        asm volatile("" : "+v"(lane_r));
        asm volatile("" : "+s"(wave_r));
        const Params *pr = pp;
        asm volatile("" : "+s"(pr));
        const Shape shape_r(pr, true);
        const Params &p = shape_r.get();
        const int64_t env_r = (int64_t)blockIdx.x * 4 + wave_r;
        // (... and the held roles: predicates derived from them would otherwise be hoisted out of the loop as SGPR masks, which
        // the kernel has no scalar registers left for -- each came back as two v_readlane per step)
        pin_roles(roles, p.range_rounds, true, p.sector_rounds == 1);
        Ctx<float> c(p, gk, smem + wave_r * p.lds_wave_bytes, lane_r, env_r, FLOW, 0);
        c.out = (int64_t)r * g.N + env_r;
        c.statics_done = stepped;
        c.pivots = Shape::kGreedyHeld;
        if (finished != 0) {
            if (lane_r == 0 && g.scalars) write_idle_row(g.scalars + c.out * 8);
            if (lane_r == 0 && g.idle_steps) g.idle_steps[env_r] += 1;      // a slot of the rollout, not an executed step
            continue;
        }
        const uint32_t tick = tick0 + (uint32_t)r;
        if (g.rotate_prio) {
            // (s_setprio takes an immediate: a two-level tree of scalar branches, not a chain of four)
            const int turn = g.rotate_prio >= 8 ? ((int)(__builtin_amdgcn_s_memtime() >> g.rotate_prio) + wave_slot) & 3 : (r + wave_slot) & 3;
            if (turn & 2) { if (turn & 1) __builtin_amdgcn_s_setprio(3); else __builtin_amdgcn_s_setprio(2); }
            else { if (turn & 1) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0); }
        }
        HEADLINE_MARK(7);      // loop overhead: from the end of the previous step to here
        if ((r & 15) == 0) headline_camera_pass(c, tick, ahead);      // (every launch starts one, whatever its first tick's parity)
        HEADLINE_MARK(8);
        StepDraws draws{0.0, 0.0};
        pin_draw_role(draws_of_lane);
        draws = step_draws(c, tick, &carry, &draws_of_lane);
        HEADLINE_MARK(0);
        headline_camera_step(c, r, ahead);
        HEADLINE_MARK(1);
        simulate_targets_held(c, draws, near, h);
        HEADLINE_MARK(2);
        uint32_t seen = 0u;
        unsigned long long sector_ballot = 0ull;
        update_view<true, true>(c, tick, S_TRANSMIT, true, roles, seen, &near, &sector_ballot);
        bool tracked; int inside;
        view_tail_held(c, sector_ballot, h, tracked, inside);
        HEADLINE_MARK(3);
        finished = assign_and_score_held(c, tick, g.scalars, h, tracked, inside);
        HEADLINE_MARK(4);
        image_targets_held(c, h, last_gw); headline_blocks<3>(c, roles, seen, zero);
        HEADLINE_MARK(5);
        headline_store<SHIFTED>(c, row_c, row_t); store_masks(c);
        wave_sync();
        stepped = true;
        HEADLINE_MARK(6);
    }
    {
        Ctx<float> c(p, gk, smem + wave * p.lds_wave_bytes, lane, env, FLOW_ANY);
        held_store(c, h);
        store_dynamic(c);
    }
}

// The two instantiations, [store_shifted]; null in a profiling build (-DMATE_PHASE_CLOCKS), whose launches all run rollout_kernel and its stamps.
using StepFn = void (*)(const Params *, const Ptrs);
StepFn headline_rollout_function(int shifted);

}  // namespace mate
