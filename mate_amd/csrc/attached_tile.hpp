// attached_tile.hpp -- the tile of the attached 16-lane-group kernels (reward_rows_kernel, selection_kernel): a 256-thread workgroup owns
// sixteen consecutive environments, a group of 16 lanes each (tid >> 4 the environment, tid & 15 the agent).  Their dynamic records are one
// contiguous stretch of HBM staged in LDS; the scalar record and the mask words arrive with one load per group (lane j: column j & 7, word j).
#pragma once
#include "engine_kernels.hpp"

namespace mate {

constexpr int kAttachedEnvsPerBlock = 16;
__host__ __device__ constexpr int attached_tile_lds_bytes(int DW) { return kAttachedEnvsPerBlock * DW * 8; }
// A tile's records, `words` consecutive doubles from its first environment's, into LDS: 512 bytes per wave and load
__device__ __forceinline__ void stage_records(double *lds, const double *src, int words, int tid) {
    for (int i = tid; i < words; i += 256) lds[i] = src[i];
}

// camera_target_view_mask: bit(c, t) = bit_ct + c * Nt + t (mate_layout.bit_camera_target) -- up to 256 bits from any origin: at most nine
// words of an environment's mask record; lane j of the group loads word j.  first word, words, the bit of (camera 0, target 0) inside the first
struct ViewWords { int first, count, origin; };
__device__ __forceinline__ ViewWords view_words(int bit_ct, int Nc, int Nt) {
    return {bit_ct >> 5, Nc * Nt > 0 ? ((bit_ct & 31) + Nc * Nt + 31) >> 5 : 0, bit_ct & 31};
}
__device__ __forceinline__ void load_view_words(uint32_t *mw, const ViewWords &v, const uint32_t *masks, int64_t env, int MW, int j) {
    if (j < v.count) mw[j] = masks[env * MW + v.first + j];
}
__device__ __forceinline__ bool view_bit(const uint32_t *mw, const ViewWords &v, int c, int t, int Nt) {
    const int bit = v.origin + c * Nt + t;
    return (mw[bit >> 5] >> (bit & 31)) & 1u;
}
// camera c's Nt bits (Nt <= 16: they straddle at most two words), bit t = target t
__device__ __forceinline__ uint32_t view_row(const uint32_t *mw, const ViewWords &v, int c, int Nt) {
    const int b = v.origin + c * Nt;
    const uint64_t w = (uint64_t)mw[b >> 5] | ((b >> 5) + 1 < v.count ? (uint64_t)mw[(b >> 5) + 1] << 32 : 0ull);
    return (uint32_t)(w >> (b & 31)) & ((1u << Nt) - 1u);
}
// `scalar`: the group's load of the step's scalar record.  done = 2: the environment waits for a batched restart, no step ran
__device__ __forceinline__ bool tile_idle(float scalar) { return __shfl(scalar, 2, 16) == 2.0f; }

}  // namespace mate
