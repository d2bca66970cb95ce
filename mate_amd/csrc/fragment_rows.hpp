// fragment_rows.hpp -- what the reference's FrameSkip wrapper (examples/utils/wrappers.py:301-323) hands the learner for one fragment of K frames,
// computed from the rollout-shaped buffers a fused K-frame launch (mate_engine_rollout_versus_greedy) has just written: the scalar records
// [K][N][8], the packed masks [K][N][MW] and the learner team's plain observation rows [K][N][A][D].  The tail of every example trainer's chain:
//   ... -> RelativeCoordinates -> RescaledObservation -> RepeatedRewardIndividualDone -> [AuxiliaryCameraRewards | AuxiliaryTargetRewards] -> FrameSkip(K)
// Not on the step path: ONE launch of its own (mate_engine_enable_fragment_rows) behind the stepping launch and ahead of the restart; the on-demand
// form (mate_engine_fragment_rows) runs it over any caller buffers.
//
// Per environment, live(f) = the scalar record of frame f does not say done = 2 (a finished or idling environment's skipped slot):
//   frames   number of live frames; `last` = the greatest live f
//   done     1 if a live frame says done = 1
//   rewards  [4] f64: the sums over the live frames, IN FRAME ORDER, of columns 0 (camera team), 1 (target team), 7 (normalised target team
//            reward) widened to f64, and the negated third (the camera side's normalised reward, environment.py:621-624)
//   info     [4] f64: the frame-order sums of coverage_rate and real_coverage_rate over `frames` (FrameSkip's 'mean' keys), mean_transport_rate and
//            num_delivered_cargoes of frame `last` (its 'last' keys)
//   shaped   [A] OutT: the sum over the live frames of that frame's AuxiliaryCameraRewards / AuxiliaryTargetRewards row -- reward_rows.hpp's
//            weighted sum (fixed key order, product then add, zero-coefficient skip), its team reduction inside each frame and its accumulating
//            store (rows += (OutT)shaped), so the result equals K accumulating reward launches of the per-step flow bit for bit.  Only the terms
//            that are functions of the scalar record and the masks exist here; soft_coverage_score, normalized_goal_distance, sparse_delivery and
//            is_colliding need the state of every frame: they read NaN, and the host refuses a non-zero coefficient for them.
//   obs      [A][D] ObsT: frame `last`'s rows, optionally through the column table: out = ((v - own x|y) if the column is a coordinate, v else;
//            +0 where the column's flag column reads 0) * scale + bias -- the operations of pack_block_xf (engine_kernels.hpp) in its order, on the
//            values the plain packer wrote, so the rows equal what the per-step flows pack under mate_engine_set_obs_transform bit for bit.
// An environment without a live frame gets frames = 0, done = 0, zero rewards / info / shaped rows, and its observation row is NOT written.
//
// Mapping: the tile of attached_tile.hpp -- sixteen environments per 256-thread workgroup, a group of 16 lanes each.  Every lane of a group walks the K
// records in frame order (one 32-byte record per frame, the same address in all sixteen lanes), so the sums exist in every lane and lane j adds
// agent j's terms; the mask words go through LDS as in reward_rows_kernel.  Then the whole workgroup copies the tile's rows, one 16-byte load and
// one 16-byte store per lane where A * D * sizeof(ObsT) is a multiple of 16 and the buffers are aligned, element by element otherwise; with a column
// table every element also reads its column's entry and, where the entry names them, the owner's x / y and the flag column (scalar loads of lines
// the tile has just read).  The result is read next by the
// learner: plain stores, which keep the lines in L2.
#pragma once
#include "reward_rows.hpp"

namespace mate {

constexpr int kFragmentRewards = 4, kFragmentInfo = 4;
constexpr int kFragmentOwnX = 13, kFragmentOwnY = 14;      // the row owner's x, y: the first two entries of its own state, behind the 13 preserved ones

template <typename ObsT> struct FragmentColumn { int32_t sub, flag; ObsT scale, bias; };      // sub: 0 none, 1 x, 2 y; flag: the column that gates, -1 none

struct FragmentArgs {
    const float *scalars;         // [K][N][8]
    const uint32_t *masks;        // [K][N][MW], or null (the mask terms then read 0)
    const void *rows;             // [K][N][A][D] ObsT: the learner team's plain rows, or null
    void *obs;                    // [N][A][D] ObsT, or null
    const void *columns;          // [D] FragmentColumn<ObsT>, or null: a plain copy
    double *rewards, *info;       // [N][4] each, or null
    uint8_t *done;                // [N], or null
    int32_t *frames;              // [N], or null
    void *shaped;                 // [N][A] OutT, or null
    const double *coef;           // [7] / [10] on the device, read at every launch
    int64_t N;
    int32_t K, team, A, D, reduction;
    int32_t bit_ct;               // mate_layout.bit_camera_target
};

// One element of the learner's row: `v` its plain value, `row` the owner's plain row, `col` the column
template <typename ObsT>
__device__ __forceinline__ ObsT fragment_element(ObsT v, const ObsT *row, int col, const FragmentColumn<ObsT> *columns) {
    if (!columns) return v;
    const FragmentColumn<ObsT> c = columns[col];
    const ObsT own = c.sub == 0 ? (ObsT)0 : row[kFragmentOwnX - 1 + c.sub];
    const bool visible = c.flag < 0 || row[c.flag] != (ObsT)0;
    const ObsT rel = v - own;
    const ObsT gated = visible ? rel : (ObsT)0;
    return gated * c.scale + c.bias;
}

template <typename ObsT, typename OutT>
__global__ __launch_bounds__(256) void fragment_rows_kernel(const Params *__restrict__ pp, const FragmentArgs a) {
    __shared__ uint32_t mask_words[kAttachedEnvsPerBlock][16];
    __shared__ int last_frame[kAttachedEnvsPerBlock];
    const Params &p = *pp;
    const int Nc = p.Nc, Nt = p.Nt;
    const int tid = threadIdx.x, el = tid >> 4, j = tid & 15;
    const int64_t e0 = (int64_t)blockIdx.x * kAttachedEnvsPerBlock;
    if (e0 >= a.N) return;
    const int ne = (int)(a.N - e0 < (int64_t)kAttachedEnvsPerBlock ? a.N - e0 : (int64_t)kAttachedEnvsPerBlock);
    const int64_t env = e0 + el;
    const bool present = el < ne;
    const bool camera = a.team == 0, agent = j < a.A;
    const bool want_shaped = a.shaped != nullptr, want_masks = want_shaped && a.masks != nullptr;
    const ViewWords vw = view_words(a.bit_ct, Nc, Nt);

    int frames = 0, last = -1, done = 0;
    double sum_cam = 0.0, sum_tgt = 0.0, sum_norm = 0.0, sum_cov = 0.0, sum_real = 0.0, last_mtr = 0.0, last_cargo = 0.0;
    OutT shaped_sum = (OutT)0;
    for (int f = 0; f < a.K; ++f) {                               // (uniform over the workgroup: the barriers below are met by every thread)
        float4 lo = make_float4(0.f, 0.f, 2.f, 0.f), hi = make_float4(0.f, 0.f, 0.f, 0.f);
        if (present) {
            const float4 *rec = reinterpret_cast<const float4 *>(a.scalars + ((int64_t)f * a.N + env) * 8);
            lo = rec[0]; hi = rec[1];
        }
        const bool live = lo.z != 2.0f;                           // (the same in all sixteen lanes of the group)
        if (want_masks) {
            if (live) load_view_words(mask_words[el], vw, a.masks + (int64_t)f * a.N * p.MW, env, p.MW, j);
            __syncthreads();
        }
        if (live) {
            frames += 1; last = f; done |= lo.z == 1.0f;
            const double s_cam = (double)lo.x, s_tgt = (double)lo.y, s_cov = (double)lo.w, s_real = (double)hi.x, s_mtr = (double)hi.y;
            sum_cam = sum_cam + s_cam; sum_tgt = sum_tgt + s_tgt; sum_norm = sum_norm + (double)hi.w;
            sum_cov = sum_cov + s_cov; sum_real = sum_real + s_real;
            last_mtr = s_mtr; last_cargo = (double)hi.z;
            if (want_shaped) {
                const uint32_t *mw = mask_words[el];
                double shaped = 0.0;
                if (camera) {
                    const int sees = want_masks && agent ? __popc(view_row(mw, vw, j, Nt)) : 0;
                    const double term[kRewardCameraTerms] = {s_cam, s_cov, s_real, s_mtr, NAN, (double)sees, 1.0};
                    MATE_REWARD_WEIGHTED_SUM(shaped, a.coef, term, kRewardCameraTerms)
                } else {
                    int seen_by = 0;
                    if (want_masks && agent) for (int c = 0; c < Nc; ++c) seen_by += view_bit(mw, vw, c, j, Nt);
                    const double term[kRewardTargetTerms] = {s_tgt, s_cov, s_real, s_mtr, NAN, NAN, NAN, seen_by > 0 ? 1.0 : 0.0, NAN, 1.0};
                    MATE_REWARD_WEIGHTED_SUM(shaped, a.coef, term, kRewardTargetTerms)
                }
                shaped = reward_reduce(shaped, agent, a.A, a.reduction);
                reward_store(&shaped_sum, shaped, REWARD_ACCUMULATE);
            }
        }
        if (want_masks) __syncthreads();                          // (the next frame's words overwrite these)
    }
    if (present) {
        if (j == 0) {
            if (a.frames) a.frames[env] = frames;
            if (a.done) a.done[env] = (uint8_t)done;
            if (a.rewards) {
                double *r = a.rewards + env * kFragmentRewards;
                r[0] = sum_cam; r[1] = sum_tgt; r[2] = sum_norm; r[3] = -sum_norm;
            }
            if (a.info) {
                double *r = a.info + env * kFragmentInfo;
                r[0] = frames > 0 ? sum_cov / (double)frames : 0.0; r[1] = frames > 0 ? sum_real / (double)frames : 0.0;
                r[2] = last_mtr; r[3] = last_cargo;
            }
            last_frame[el] = last;
        }
        if (want_shaped && agent) reinterpret_cast<OutT *>(a.shaped)[env * a.A + j] = shaped_sum;
    }
    if (!a.obs || !a.rows) return;                                // (uniform)
    __syncthreads();

    // the tile's rows of frame `last`, by the whole workgroup
    const int row_elems = a.A * a.D;
    const ObsT *src = reinterpret_cast<const ObsT *>(a.rows);
    ObsT *dst = reinterpret_cast<ObsT *>(a.obs);
    const FragmentColumn<ObsT> *columns = reinterpret_cast<const FragmentColumn<ObsT> *>(a.columns);
    constexpr int W = 16 / (int)sizeof(ObsT);
    const bool wide = (row_elems % W) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
    if (wide) {
        typedef ObsT vec_t __attribute__((ext_vector_type(W)));
        const int row_vecs = row_elems / W;
        for (int i = tid; i < ne * row_vecs; i += 256) {
            const int e = i / row_vecs, v = i - e * row_vecs;
            const int f = last_frame[e];
            if (f < 0) continue;
            const ObsT *row = src + ((int64_t)f * a.N + e0 + e) * row_elems;
            vec_t out = reinterpret_cast<const vec_t *>(row)[v];
            if (columns) {
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    const int x = v * W + k, owner = x / a.D;
                    out[k] = fragment_element(out[k], row + owner * a.D, x - owner * a.D, columns);
                }
            }
            reinterpret_cast<vec_t *>(dst + (e0 + e) * row_elems)[v] = out;
        }
    } else {
        for (int i = tid; i < ne * row_elems; i += 256) {
            const int e = i / row_elems, x = i - e * row_elems;
            const int f = last_frame[e];
            if (f < 0) continue;
            const ObsT *row = src + ((int64_t)f * a.N + e0 + e) * row_elems;
            const int owner = x / a.D;
            dst[(e0 + e) * row_elems + x] = fragment_element(row[x], row + owner * a.D, x - owner * a.D, columns);
        }
    }
}

}  // namespace mate
