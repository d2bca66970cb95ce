// frame_rows.hpp -- the FrameSkip fragment of fragment_rows.hpp built FRAME BY FRAME: one small launch behind each per-step call of a learner-versus-opponents
// flow (mate_engine_step_versus_greedy) folds that call's frame into the fragment tensors, so a fragment of K frames is K per-step calls -- any opponent the
// per-step flows have (Heuristic, Naive, Random, mixtures, channels) and every shaping term, since the per-step reward launch sees every frame's state.
// Not on the step path: a launch of its own (mate_engine_enable_frame_fragments) behind the stepping launch, the reward launch and the selection metrics and
// ahead of the restart; the on-demand form (mate_engine_frame_fragment) runs it over any caller buffers.  Emitted by opponent_kernels.hip.
//
// The launch reads the call's own scalar records [N][8] f32, the learner team's rows [N][A][D] ObsT (the packer's fused transform already applied:
// mate_engine_set_obs_transform) and, for the shaped rows, the learner team's reward rows [N][A] of the overwrite-mode reward launch of the same call.
// live = the record's column 2 does not say 2 (an idling environment's skipped slot).  `phase` f = 0 .. K - 1, per environment:
//   f = 0        frames = 0, done = 0, rewards = 0, the two coverage sums and the two last-frame columns = 0, shaped = 0, restarted = 0 -- stores, not adds:
//                no memset node in front
//   live         frames += 1; done |= (column 2 == 1); rewards[0..2] = rewards[0..2] + (f64) columns 0, 1, 7 and rewards[3] = -rewards[2] (the sum of
//                the negated column: IEEE addition is symmetric in sign, and the fused fragment stores the negated sum); info[0..1] += columns 3, 4;
//                info[2..3] = columns 5, 6; shaped[a] = (OutT)(shaped[a] + row[a]) -- what accumulating reward launches leave over zeroed rows
//   f = K - 1    info[0..1] /= frames (0 where frames = 0): the fused fragment's frame-order sum / frames
//   rows         on the environment's last live frame of the fragment (column 2 == 1, or live and f = K - 1) the learner team's rows go to obs[e], a plain
//                copy; an environment without a live frame keeps its obs row unwritten
// The same f64 adds in the same order as fragment_rows_kernel's registers make, through memory: bit-identical to the fused fragment.
// `closes` (the second form, behind the restart launch of a call that closes an interval, where first rows were asked for): for every environment whose
// record of this call says column 2 != 0 -- finished in this frame, or idling since: exactly what the restart has restarted --
//   final_obs[e] <- obs[e] (where asked for), then obs[e] <- rows[e] (the restart has just made them the new episode's first rows), restarted[e] = 1.
//
// Mapping: the tile of attached_tile.hpp -- sixteen environments per 256-thread workgroup, a group of 16 lanes each.  Lane 0 of a group carries the scalars,
// lane j agent j's shaped value; a per-environment flag in LDS says whose rows move, and the whole workgroup moves them, one 16-byte load and one 16-byte
// store per lane where A * D * sizeof(ObsT) is a multiple of 16 and the buffers are aligned, element by element otherwise.  Plain stores: the learner
// reads the rows next.  Every offset an environment index enters is 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mate {

constexpr int kFrameEnvsPerBlock = 16;       // (kAttachedEnvsPerBlock: attached_tile.hpp)

struct FrameArgs {
    const float *scalars;         // [N][8] of this call
    const void *rows;             // [N][A][D] ObsT: the learner team's rows of this call
    const void *reward_rows;      // [N][A] OutT: the learner team's overwrite-mode reward rows of this call, or null
    void *obs, *final_obs;        // [N][A][D] ObsT each, or null
    uint8_t *restarted;           // [N], or null
    double *rewards, *info;       // [N][4] each, or null
    uint8_t *done;                // [N], or null
    int32_t *frames;              // [N] (required with info)
    void *shaped;                 // [N][A] OutT, or null
    int64_t N;
    int32_t phase, K, closes, A, D, shaped_f64;
};

template <typename OutT>
__device__ __forceinline__ void frame_shaped(const FrameArgs &a, int64_t at, bool first, bool live) {
    OutT *dst = reinterpret_cast<OutT *>(a.shaped) + at;
    OutT sum = first ? (OutT)0 : *dst;
    if (live) sum = (OutT)(sum + reinterpret_cast<const OutT *>(a.reward_rows)[at]);
    if (first || live) *dst = sum;
}

template <typename ObsT>
__global__ __launch_bounds__(256) void fragment_frame_kernel(const FrameArgs a) {
    __shared__ int moves[kFrameEnvsPerBlock];
    const int tid = threadIdx.x, el = tid >> 4, j = tid & 15;
    const int64_t e0 = (int64_t)blockIdx.x * kFrameEnvsPerBlock;
    if (e0 >= a.N) return;
    const int ne = (int)(a.N - e0 < (int64_t)kFrameEnvsPerBlock ? a.N - e0 : (int64_t)kFrameEnvsPerBlock);
    const int64_t env = e0 + el;
    const bool present = el < ne, first = a.phase == 0, closing = a.phase == a.K - 1;
    const bool want_rows = a.obs != nullptr && a.rows != nullptr;

    if (present) {
        const float4 *rec = reinterpret_cast<const float4 *>(a.scalars + env * 8);
        const float flag = a.scalars[env * 8 + 2];                   // (the same address in all sixteen lanes of the group)
        const bool live = flag != 2.0f;
        if (a.closes) {
            if (j == 0) {
                moves[el] = flag != 0.0f;
                if (a.restarted && flag != 0.0f) a.restarted[env] = 1;
            }
        } else {
            if (j == 0) {
                const float4 lo = rec[0], hi = rec[1];
                int frames = (first || !a.frames) ? 0 : a.frames[env];
                if (live) frames += 1;
                if (a.frames) a.frames[env] = frames;
                if (a.done) a.done[env] = (uint8_t)(((first ? 0 : a.done[env]) | (live && lo.z == 1.0f)) != 0);
                if (a.restarted && first) a.restarted[env] = 0;
                if (a.rewards) {
                    double *r = a.rewards + env * 4;
                    double sum_cam = first ? 0.0 : r[0], sum_tgt = first ? 0.0 : r[1], sum_norm = first ? 0.0 : r[2];
                    if (live) { sum_cam = sum_cam + (double)lo.x; sum_tgt = sum_tgt + (double)lo.y; sum_norm = sum_norm + (double)hi.w; }
                    r[0] = sum_cam; r[1] = sum_tgt; r[2] = sum_norm; r[3] = -sum_norm;
                }
                if (a.info) {
                    double *r = a.info + env * 4;
                    double sum_cov = first ? 0.0 : r[0], sum_real = first ? 0.0 : r[1], last_mtr = first ? 0.0 : r[2], last_cargo = first ? 0.0 : r[3];
                    if (live) { sum_cov = sum_cov + (double)lo.w; sum_real = sum_real + (double)hi.x; last_mtr = (double)hi.y; last_cargo = (double)hi.z; }
                    if (closing) { sum_cov = frames > 0 ? sum_cov / (double)frames : 0.0; sum_real = frames > 0 ? sum_real / (double)frames : 0.0; }
                    r[0] = sum_cov; r[1] = sum_real; r[2] = last_mtr; r[3] = last_cargo;
                }
                moves[el] = live && (lo.z == 1.0f || closing);
            }
            if (a.shaped && j < a.A) {
                if (a.shaped_f64) frame_shaped<double>(a, env * a.A + j, first, live);
                else frame_shaped<float>(a, env * a.A + j, first, live);
            }
        }
    }
    if (!want_rows) return;                                       // (uniform)
    __syncthreads();

    // the flagged environments' rows, by the whole workgroup: thread i handles the same elements in both copies of the second form
    const int row_elems = a.A * a.D;
    const ObsT *src = reinterpret_cast<const ObsT *>(a.rows);
    ObsT *dst = reinterpret_cast<ObsT *>(a.obs);
    ObsT *keep = a.closes ? reinterpret_cast<ObsT *>(a.final_obs) : nullptr;
    constexpr int W = 16 / (int)sizeof(ObsT);
    const bool wide = (row_elems % W) == 0 &&
                      ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(keep)) & 15u) == 0;
    if (wide) {
        typedef ObsT vec_t __attribute__((ext_vector_type(W)));
        const int row_vecs = row_elems / W;
        for (int i = tid; i < ne * row_vecs; i += 256) {
            const int e = i / row_vecs, v = i - e * row_vecs;
            if (!moves[e]) continue;
            const int64_t at = (e0 + e) * row_elems;
            if (keep) reinterpret_cast<vec_t *>(keep + at)[v] = reinterpret_cast<const vec_t *>(dst + at)[v];
            reinterpret_cast<vec_t *>(dst + at)[v] = reinterpret_cast<const vec_t *>(src + at)[v];
        }
    } else {
        for (int i = tid; i < ne * row_elems; i += 256) {
            const int e = i / row_elems, x = i - e * row_elems;
            if (!moves[e]) continue;
            const int64_t at = (e0 + e) * row_elems + x;
            if (keep) keep[at] = dst[at];
            dst[at] = src[at];
        }
    }
}

// (opponent_kernels.hip) `obs_f64`: the instance
hipError_t launch_fragment_frame(bool obs_f64, unsigned blocks, hipStream_t stream, const FrameArgs &a);

}  // namespace mate
