// reward_rows.hpp -- the shaped per-agent rewards of every environment: the reference's AuxiliaryCameraRewards
// (wrappers/auxiliary_camera_rewards.py:110-176) and AuxiliaryTargetRewards (wrappers/auxiliary_target_rewards.py:128-203) with
// one coefficient per term, as ONE launch over the records a step has just left in HBM -- the last wrapper of every example
// trainer's chain (examples/*/camera/config.py, examples/*/target/config.py).  Not on the step path: a launch of its own
// (mate_engine_enable_reward_rows), enqueued behind every stepping launch and AHEAD of the restart of finished episodes, so that
// the rows describe the step the scalar record describes, the terminal one included.
//
// Terms, in the order of the coefficient tables (a term whose coefficient is exactly 0 is not added: a NaN soft coverage
// value of an environment without an outer table must not leak into a sum that does not ask for it):
//   camera [7]:  raw_reward (scalar column 0) | coverage_rate (3) | real_coverage_rate (4) | mean_transport_rate (5) |
//                soft_coverage_score | num_tracked | baseline
//   target [10]: raw_reward (scalar column 1) | coverage_rate | real_coverage_rate | mean_transport_rate |
//                normalized_goal_distance | sparse_delivery | soft_coverage_score | is_tracked | is_colliding | baseline
// The four shared terms are the f32 step record widened to f64; the sum runs in that order, product then add (-ffp-contract=off).
//
// Mapping: the tile of attached_tile.hpp; lane j of a group is target j AND camera j (the engine takes at most sixteen of each).
// The scalar record is handed round by shuffles, the mask words through LDS; the reductions over an environment's agents are
// four-stage butterflies inside the group.
#pragma once
#include "attached_tile.hpp"

namespace mate {

constexpr int kRewardCameraTerms = 7, kRewardTargetTerms = 10;
enum RewardMode : int32_t { REWARD_OVERWRITE = 0, REWARD_ACCUMULATE = 1, REWARD_SNAPSHOT = 2 };
enum RewardReduction : int32_t { REDUCE_NONE = 0, REDUCE_MEAN = 1, REDUCE_SUM = 2, REDUCE_MAX = 3, REDUCE_MIN = 4 };

struct RewardArgs {
    const float *scalars;         // [N][8] of the step the rows describe
    const uint32_t *masks;        // [N][MW] of that step
    int32_t *snapshot;            // [N][Nt + 1]: the goals the previous launch saw, then its episode number
    void *cam_rows, *tgt_rows;    // [N][Nc] / [N][Nt] OutT, either may be null
    double *cam_terms, *tgt_terms;            // optional [N][Nc][7] / [N][Nt][10]
    const double *cam_coef, *tgt_coef;        // [7] / [10], read at every launch
    const double *soft_matrix, *soft_scores;  // [N][Nc][Nt] / [N][Nc] of soft_coverage_kernel on the same records, or null
    int32_t cam_reduction, tgt_reduction;
    int32_t mode;
    int32_t bit_ct;               // mate_layout.bit_camera_target
};

// over the sixteen lanes of an environment's group; lanes that hold no agent carry the identity
__device__ __forceinline__ double group16_reduce(double v, int how) {
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, 16);
        v = how == REDUCE_MAX ? (o > v ? o : v) : how == REDUCE_MIN ? (o < v ? o : v) : v + o;
    }
    return v;
}
__device__ __forceinline__ double reward_reduce(double mine, bool agent, int agents, int how) {
    if (how == REDUCE_NONE) return mine;
    const double identity = how == REDUCE_MAX ? -INFINITY : how == REDUCE_MIN ? INFINITY : 0.0;
    const double all = group16_reduce(agent ? mine : identity, how);
    return how == REDUCE_MEAN ? all / (double)agents : all;
}

// A frame's shaped value ahead of the team reduction: the terms in the order of the coefficient table, product then add; a term whose coefficient
// is exactly 0 is not added.  ONE text for reward_rows_kernel and fragment_rows_kernel (fragment_rows.hpp); a macro, not a function, so that
// reward_rows_kernel compiles to the instructions it had before the loop was shared (as an inlined function the adds came out with swapped operands).
#define MATE_REWARD_WEIGHTED_SUM(shaped, coef, term, K)          \
    _Pragma("unroll") for (int k = 0; k < (K); ++k) {            \
        const double c = (coef)[k];                              \
        if (c != 0.0) shaped = shaped + c * (term)[k];           \
    }

template <typename OutT>
__device__ __forceinline__ void reward_store(OutT *row, double shaped, int mode) {
    *row = mode == REWARD_ACCUMULATE ? (OutT)(*row + (OutT)shaped) : (OutT)shaped;
}

template <typename OutT>
__global__ __launch_bounds__(256) void reward_rows_kernel(const Params *__restrict__ pp, const Ptrs g, const RewardArgs a) {
    extern __shared__ __align__(16) unsigned char reward_lds[];
    __shared__ uint32_t mask_words[kAttachedEnvsPerBlock][16];
    const Params &p = *pp;
    const int Nc = p.Nc, Nt = p.Nt, DW = p.DW;
    const int tid = threadIdx.x, el = tid >> 4, j = tid & 15;
    const int64_t e0 = (int64_t)blockIdx.x * kAttachedEnvsPerBlock;
    if (e0 >= g.N) return;
    const int ne = (int)(g.N - e0 < (int64_t)kAttachedEnvsPerBlock ? g.N - e0 : (int64_t)kAttachedEnvsPerBlock);
    double *dy = reinterpret_cast<double *>(reward_lds);
    stage_records(dy, g.dyn + e0 * DW, ne * DW, tid);
    const int64_t env = e0 + el;
    const bool live = el < ne, step = a.mode != REWARD_SNAPSHOT;
    const ViewWords vw = view_words(a.bit_ct, Nc, Nt);
    float scalar = 0.f;
    if (live && step) {
        scalar = a.scalars[env * 8 + (j & 7)];
        load_view_words(mask_words[el], vw, a.masks, env, p.MW, j);
    }
    __syncthreads();
    if (!live) return;

    const double *d = dy + el * DW;
    const int32_t *di = reinterpret_cast<const int32_t *>(d + p.DF);
    const bool is_tgt = j < Nt, is_cam = j < Nc;
    const int gw = is_tgt ? di[j * TI_STRIDE + TI_GW] : 0;
    const int goal = (gw & 0xff) - 1;
    const int episode = di[Nt * TI_STRIDE + EI_EPISODE];
    int32_t *snap = a.snapshot + env * (Nt + 1);
    if (!step) {                                                   // snapshot-only: behind a restart / reset / import
        if (is_tgt) snap[j] = goal;
        if (j == 0) snap[Nt] = episode;
        return;
    }
    const double s_cam = (double)__shfl(scalar, 0, 16), s_tgt = (double)__shfl(scalar, 1, 16), s_cov = (double)__shfl(scalar, 3, 16),
                 s_real = (double)__shfl(scalar, 4, 16), s_mtr = (double)__shfl(scalar, 5, 16);
    const bool idle = tile_idle(scalar);
    OutT *cam_row = reinterpret_cast<OutT *>(a.cam_rows), *tgt_row = reinterpret_cast<OutT *>(a.tgt_rows);
    if (idle) {                                                    // contributes nothing; its snapshot stays
        if (a.mode == REWARD_OVERWRITE) {
            if (cam_row && is_cam) cam_row[env * Nc + j] = (OutT)0;
            if (tgt_row && is_tgt) tgt_row[env * Nt + j] = (OutT)0;
            if (a.cam_terms && is_cam) for (int k = 0; k < kRewardCameraTerms; ++k) a.cam_terms[(env * Nc + j) * kRewardCameraTerms + k] = 0.0;
            if (a.tgt_terms && is_tgt) for (int k = 0; k < kRewardTargetTerms; ++k) a.tgt_terms[(env * Nt + j) * kRewardTargetTerms + k] = 0.0;
        }
        return;
    }

    // one pass over the other team: as target j the cameras that see it, as camera j the targets it sees
    const bool soft_t = tgt_row && a.soft_matrix;
    int seen_by = 0, sees = 0;
    double soft_sum = 0.0, soft_max = -INFINITY;
    const uint32_t *mw = mask_words[el];
    for (int k = 0; k < (Nc > Nt ? Nc : Nt); ++k) {
        if (is_tgt && k < Nc) {
            const bool seen = view_bit(mw, vw, k, j, Nt);
            seen_by += seen;
            if (soft_t) {                                          // auxiliary_target_rewards.py:146-158
                const double m = a.soft_matrix[(env * Nc + k) * Nt + j];
                if (seen) soft_sum += m;
                soft_max = m > soft_max ? m : soft_max;
            }
        }
        if (is_cam && k < Nt) sees += view_bit(mw, vw, j, k, Nt);
    }

    if (tgt_row) {
        double term[kRewardTargetTerms];
        term[0] = s_tgt; term[1] = s_cov; term[2] = s_real; term[3] = s_mtr;
        {   // :131-143 -- distance to the goal warehouse's rim, else to the nearest non-empty one, else half the terrain
            const double tx = is_tgt ? d[2 * Nc + j] : 0.0, ty = is_tgt ? d[2 * Nc + Nt + j] : 0.0;
            const int empty = (gw >> 16) & 0xf;
            double to_goal = 0.0, nearest = INFINITY;
#pragma unroll
            for (int w = 0; w < 4; ++w) {                          // constants.py:17: (+,+) (-,+) (-,-) (+,-) x 925
                const double dx = tx - ((w == 1 || w == 2) ? -925.0 : 925.0), dyw = ty - (w >= 2 ? -925.0 : 925.0);
                const double away = sqrt(dx * dx + dyw * dyw) - 75.0;
                const double rim = away > 0.0 ? away : 0.0;
                to_goal = goal == w ? rim : to_goal;
                if (!((empty >> w) & 1)) nearest = rim < nearest ? rim : nearest;
            }
            const double dist = goal >= 0 ? to_goal : empty != 0xf ? nearest : 1000.0;
            term[4] = dist / 2000.0;
        }
        const int before = is_tgt ? snap[j] : -1;
        const int episode_before = snap[Nt];
        term[5] = (goal != before && before >= 0 && episode == episode_before) ? 1.0 : 0.0;       // environment.py:1320-1322
        term[6] = !a.soft_matrix ? NAN : seen_by > 0 ? soft_sum : tanh(soft_max);      // (not computed: a sum that asks for it says so)
        term[7] = seen_by > 0 ? 1.0 : 0.0;
        term[8] = (double)((gw >> 24) & 1);
        term[9] = 1.0;
        double shaped = 0.0;
        MATE_REWARD_WEIGHTED_SUM(shaped, a.tgt_coef, term, kRewardTargetTerms)
        shaped = reward_reduce(shaped, is_tgt, Nt, a.tgt_reduction);
        if (is_tgt) {
            reward_store(tgt_row + env * Nt + j, shaped, a.mode);
            if (a.tgt_terms) {
#pragma unroll
                for (int k = 0; k < kRewardTargetTerms; ++k) a.tgt_terms[(env * Nt + j) * kRewardTargetTerms + k] = term[k];
            }
        }
    }
    if (cam_row) {
        double term[kRewardCameraTerms];
        term[0] = s_cam; term[1] = s_cov; term[2] = s_real; term[3] = s_mtr;
        term[4] = !a.soft_scores ? NAN : is_cam ? a.soft_scores[env * Nc + j] : 0.0;
        term[5] = (double)sees;
        term[6] = 1.0;
        double shaped = 0.0;
        MATE_REWARD_WEIGHTED_SUM(shaped, a.cam_coef, term, kRewardCameraTerms)
        shaped = reward_reduce(shaped, is_cam, Nc, a.cam_reduction);
        if (is_cam) {
            reward_store(cam_row + env * Nc + j, shaped, a.mode);
            if (a.cam_terms) {
#pragma unroll
                for (int k = 0; k < kRewardCameraTerms; ++k) a.cam_terms[(env * Nc + j) * kRewardCameraTerms + k] = term[k];
            }
        }
    }
    // the goals and the episode the next launch measures sparse_delivery against
    if (is_tgt) snap[j] = goal;
    if (j == 0) snap[Nt] = episode;
}

}  // namespace mate
