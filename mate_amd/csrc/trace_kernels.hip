// trace_kernels.hip -- comm_trace_kernel and its launch function (trace_rows.hpp describes them), as a translation unit of its own: its
// kernel-resource remarks are kept apart from every pinned record (mate_amd/build.py: lib/trace_resources.json).
#include <hip/hip_runtime.h>
#include "trace_rows.hpp"

namespace mate {

enum TraceFlag : uint32_t { TRACE_LIVE = 1u, TRACE_KEPT = 2u /* << team */, TRACE_ROUTED = 8u /* << team */ };

// one byte of the matrix through the step: the countdown (from zero where the matrix belongs to another episode), then the mark
__device__ __forceinline__ uint32_t trace_byte(uint32_t remaining, bool kept, bool marked, uint32_t duration) {
    const uint32_t left = kept && remaining > 0u ? remaining - 1u : 0u;
    return marked ? duration : left;
}

__global__ __launch_bounds__(256) void comm_trace_kernel(const Params *__restrict__ pp, const TraceArgs a) {
    __shared__ uint32_t flags[kAttachedEnvsPerBlock];
    const Params &p = *pp;
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * kAttachedEnvsPerBlock;
    if (e0 >= a.N) return;
    const int present = (int)(a.N - e0 < kAttachedEnvsPerBlock ? a.N - e0 : kAttachedEnvsPerBlock);
    if (tid < kAttachedEnvsPerBlock) {
        uint32_t f = 0u;
        if (tid < present) {
            const int64_t env = e0 + tid;
            const int32_t *ei = reinterpret_cast<const int32_t *>(a.dyn + env * p.DW + p.DF) + p.Nt * TI_STRIDE;
            const int32_t tick = ei[EI_TICK], episode = ei[EI_EPISODE];
            const bool live = !(a.freeze_done && ei[EI_DONE] != 0);
            f = live ? TRACE_LIVE : 0u;
            for (int team = 0; team < 2; ++team) {
                const TraceTeam &t = a.team[team];
                if (t.n == 0) continue;
                if (t.tags[env] == episode) f |= TRACE_KEPT << team;
                else if (live) t.tags[env] = episode;
                if (t.step_edges && t.message_tags[env * 2] == tick && t.message_tags[env * 2 + 1] == episode) f |= TRACE_ROUTED << team;
            }
        }
        flags[tid] = f;
    }
    __syncthreads();
    const uint32_t duration = (uint32_t)a.duration;
    for (int team = 0; team < 2; ++team) {
        const TraceTeam &t = a.team[team];
        if (t.n == 0) continue;
        const int nn = t.n * t.n;
        const int64_t base = e0 * nn;
        const int run = present * nn;                          // bytes of this tile: every offset below stays inside [0, N n n)
        if ((nn & 15) == 0) {
            for (int piece = tid; piece < (run >> 4); piece += 256) {
                const uint32_t f = flags[(piece << 4) / nn];
                if (!(f & TRACE_LIVE)) continue;
                const bool kept = (f >> team) & TRACE_KEPT, routed = (f >> team) & TRACE_ROUTED;
                const int64_t at = base + ((int64_t)piece << 4);
                uint4 r = *reinterpret_cast<const uint4 *>(t.remaining + at);
                uint4 d = make_uint4(0u, 0u, 0u, 0u);
                if (t.delivered) d = *reinterpret_cast<const uint4 *>(t.delivered + at);
                uint32_t rw[4] = {r.x, r.y, r.z, r.w};
                const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    int4 m = make_int4(0, 0, 0, 0);
                    if (routed) m = *reinterpret_cast<const int4 *>(t.step_edges + at + 4 * w);
                    const int32_t mw[4] = {m.x, m.y, m.z, m.w};
                    uint32_t out = 0u;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const bool marked = ((dw[w] >> (8 * b)) & 0xffu) != 0u || mw[b] > 0;
                        out |= trace_byte((rw[w] >> (8 * b)) & 0xffu, kept, marked, duration) << (8 * b);
                    }
                    rw[w] = out;
                }
                *reinterpret_cast<uint4 *>(t.remaining + at) = make_uint4(rw[0], rw[1], rw[2], rw[3]);
            }
        } else {
            for (int b = tid; b < run; b += 256) {
                const uint32_t f = flags[b / nn];
                if (!(f & TRACE_LIVE)) continue;
                const bool kept = (f >> team) & TRACE_KEPT, routed = (f >> team) & TRACE_ROUTED;
                const int64_t at = base + b;
                const bool marked = (t.delivered && t.delivered[at] != 0) || (routed && t.step_edges[at] > 0);
                t.remaining[at] = (uint8_t)trace_byte(t.remaining[at], kept, marked, duration);
            }
        }
    }
}

// mate_engine_set_comm_trace: a caller's matrices in place of the engine's, tagged with the environments' episode numbers as they are
__global__ __launch_bounds__(256) void trace_plant_kernel(const Params *__restrict__ pp, const double *__restrict__ dyn, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                          int32_t *__restrict__ tags, const int64_t N, const int32_t nn) {
    const Params &p = *pp;
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * kAttachedEnvsPerBlock;
    if (e0 >= N) return;
    const int present = (int)(N - e0 < kAttachedEnvsPerBlock ? N - e0 : kAttachedEnvsPerBlock);
    if (tid < present) tags[e0 + tid] = (reinterpret_cast<const int32_t *>(dyn + (e0 + tid) * p.DW + p.DF) + p.Nt * TI_STRIDE)[EI_EPISODE];
    for (int b = tid; b < present * nn; b += 256) dst[e0 * nn + b] = src[e0 * nn + b];
}

hipError_t launch_trace_plant(unsigned blocks, hipStream_t stream, const Params *params, const double *dyn, const uint8_t *src, uint8_t *dst, int32_t *tags, int64_t N, int32_t nn) {
    hipLaunchKernelGGL(trace_plant_kernel, dim3(blocks), dim3(256), 0, stream, params, dyn, src, dst, tags, N, nn);
    return hipGetLastError();
}

hipError_t launch_comm_trace(unsigned blocks, hipStream_t stream, const Params *params, const TraceArgs &a) {
    hipLaunchKernelGGL(comm_trace_kernel, dim3(blocks), dim3(256), 0, stream, params, a);
    return hipGetLastError();
}

}  // namespace mate
