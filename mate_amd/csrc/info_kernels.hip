// info_kernels.hip -- info_rows_kernel and its launch function (info_rows.hpp describes them), as a translation unit of its own: its
// kernel-resource remarks are kept apart from the other units' (mate_amd/build.py: lib/kernel_resources_info.json).
#include <hip/hip_runtime.h>
#include "info_rows.hpp"

namespace mate {

// OR over the sixteen lanes of an environment's group; lanes that hold no agent carry 0
__device__ __forceinline__ uint32_t info_group_or(uint32_t v) {
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) v |= __shfl_xor(v, off, 16);
    return v;
}

// One output of a tile leaves LDS: `ne` rows of `row` doubles, contiguous from `dst` (16-byte aligned: a tile starts at a multiple of sixteen rows), two
// doubles per lane and store where both belong to environments this launch writes (`writes`), one where only one does.
__device__ __forceinline__ void info_store_tile(double *dst, const double *stage, int row, int ne, const int32_t *writes, int tid) {
    const int count = ne * row;
    for (int i = 2 * tid; i < count; i += 512) {
        const bool first = writes[i / row] != 0, second = i + 1 < count && writes[(i + 1) / row] != 0;
        if (first && second) *reinterpret_cast<double2 *>(dst + i) = make_double2(stage[i], stage[i + 1]);
        else if (first) dst[i] = stage[i];
        else if (second) dst[i + 1] = stage[i + 1];
    }
}

__global__ __launch_bounds__(256) void info_rows_kernel(const Params *__restrict__ pp, const InfoArgs a) {
    extern __shared__ __align__(16) unsigned char info_lds[];
    __shared__ uint32_t mask_words[kAttachedEnvsPerBlock][16];
    __shared__ int32_t writes[kAttachedEnvsPerBlock];              // the environment's rows are rewritten by this launch
    const Params &p = *pp;
    const int Nc = p.Nc, Nt = p.Nt, DW = p.DW;
    const int tid = threadIdx.x, el = tid >> 4, j = tid & 15;
    const int64_t e0 = (int64_t)blockIdx.x * kAttachedEnvsPerBlock;
    if (e0 >= a.N) return;
    const int ne = (int)(a.N - e0 < (int64_t)kAttachedEnvsPerBlock ? a.N - e0 : (int64_t)kAttachedEnvsPerBlock);
    double *dy = reinterpret_cast<double *>(info_lds);
    double *tgt_stage = dy + kAttachedEnvsPerBlock * DW, *cam_stage = tgt_stage + kAttachedEnvsPerBlock * Nt * kInfoTargetColumns,
           *cargo_stage = cam_stage + kAttachedEnvsPerBlock * Nc * kInfoCameraColumns;
    stage_records(dy, a.dyn + e0 * DW, ne * DW, tid);
    const int64_t env = e0 + el;
    const bool live = el < ne, step = a.mode == INFO_STEP, snapshot_only = a.mode == INFO_SNAPSHOT;
    const bool have_masks = a.masks != nullptr && !snapshot_only;
    const ViewWords vw = view_words(a.bit_ct, Nc, Nt);
    float scalar = 0.f;
    uint32_t sensing = 0u;                                         // as target j: bit c = target j senses camera c
    if (live && step) scalar = a.scalars[env * 8 + (j & 7)];
    if (live && have_masks) {
        load_view_words(mask_words[el], vw, a.masks, env, p.MW, j);
        if (j < Nt && Nc > 0) {                                    // row j of the target rows: Nc <= 16 bits from bit_tr + j NJ, in at most two words
            const int b = a.bit_tr + j * p.NJ, w = b >> 5;
            const uint32_t *m = a.masks + env * p.MW;
            const uint64_t lo = m[w], hi = w + 1 < p.MW ? m[w + 1] : 0u;
            sensing = (uint32_t)((lo | (hi << 32)) >> (b & 31)) & ((1u << Nc) - 1u);
        }
    }
    __syncthreads();

    const bool idle = tile_idle(scalar) && step;                   // done = 2: no step ran; rows and snapshot stay
    const bool rows = live && !snapshot_only && !idle;
    if (j == 0) writes[el] = rows;
    const bool is_tgt = live && j < Nt, is_cam = live && j < Nc;
    const double *d = dy + el * DW;
    const int32_t *di = reinterpret_cast<const int32_t *>(d + p.DF);
    const int gw = is_tgt ? di[j * TI_STRIDE + TI_GW] : 0;
    const int goal = (gw & 0xff) - 1;
    const int episode = live ? di[Nt * TI_STRIDE + EI_EPISODE] : 0;

    uint32_t seeing = 0u;                                          // as camera j: bit t = camera j sees target t
    if (is_cam && have_masks) seeing = view_row(mask_words[el], vw, j, Nt);
    const uint32_t tracked = info_group_or(seeing), sensed = info_group_or(sensing);      // bit t: is_tracked(t); bit c: is_sensed(c)

    if (rows && a.tgt_rows && is_tgt) {
        double *o = tgt_stage + (el * Nt + j) * kInfoTargetColumns;
        const double tx = d[2 * Nc + j], ty = d[2 * Nc + Nt + j];
        double to_goal = 1000.0;                                   // environment.py:1308: TERRAIN_WIDTH / 2 without a goal
#pragma unroll
        for (int w = 0; w < 4; ++w) {                              // constants.py:17: (+,+) (-,+) (-,-) (+,-) x 925
            const double dx = tx - ((w == 1 || w == 2) ? -925.0 : 925.0), dyw = ty - (w >= 2 ? -925.0 : 925.0);
            const double away = sqrt(dx * dx + dyw * dyw) - 75.0;
            const double rim = away > 0.0 ? away : 0.0;
            to_goal = goal == w ? rim : to_goal;
            o[2 + w] = rim;
        }
        double done = NAN;                                         // on demand, or a multi-frame call
        if (step && !a.done_nan) {
            const int32_t *snap = a.snapshot + env * (Nt + 1);
            const int before = snap[j], episode_before = snap[Nt];
            done = (goal != before && before >= 0 && episode == episode_before) ? 1.0 : 0.0;      // environment.py:1320-1322
        }
        o[0] = (double)goal; o[1] = to_goal; o[6] = done;
        o[7] = have_masks ? (double)((tracked >> j) & 1u) : NAN;
        o[8] = (double)((gw >> 24) & 1);
    }
    if (rows && a.cam_rows && is_cam) {
        double *o = cam_stage + (el * Nc + j) * kInfoCameraColumns;
        o[0] = have_masks ? (double)__popc(seeing) : NAN;
        o[1] = have_masks ? (double)((sensed >> j) & 1u) : NAN;
    }
    if (rows && a.cargo_rows) {                                    // lane j: column j, and column 16 + j below 8
        const int32_t *ei = di + Nt * TI_STRIDE;
        double *o = cargo_stage + el * kInfoCargoColumns;
        int v;
        if (j < 4) { const int32_t *r = ei + EI_REMAINING + 4 * j; v = r[0] + r[1] + r[2] + r[3]; }
        else if (j < 8) v = ei[EI_AWAITING + j - 4];
        else v = ei[EI_REMAINING + j - 8];
        o[j] = (double)v;
        if (j < 8) o[16 + j] = (double)ei[EI_REMAINING + 8 + j];
    }
    // the goals and the episode the next step's individual_done is measured against
    if (live && (snapshot_only || (step && !idle))) {
        int32_t *snap = a.snapshot + env * (Nt + 1);
        if (is_tgt) snap[j] = goal;
        if (j == 0) snap[Nt] = episode;
    }
    if (snapshot_only) return;                                     // (the same in every lane of the launch)
    __syncthreads();

    if (a.tgt_rows) info_store_tile(a.tgt_rows + e0 * Nt * kInfoTargetColumns, tgt_stage, Nt * kInfoTargetColumns, ne, writes, tid);
    if (a.cam_rows && Nc > 0) info_store_tile(a.cam_rows + e0 * Nc * kInfoCameraColumns, cam_stage, Nc * kInfoCameraColumns, ne, writes, tid);
    if (a.cargo_rows) info_store_tile(a.cargo_rows + e0 * kInfoCargoColumns, cargo_stage, kInfoCargoColumns, ne, writes, tid);
}

hipError_t launch_info_rows(unsigned blocks, size_t lds, hipStream_t stream, const Params *params, const InfoArgs &a) {
    hipLaunchKernelGGL(info_rows_kernel, dim3(blocks), dim3(256), lds, stream, params, a);
    return hipGetLastError();
}

}  // namespace mate
