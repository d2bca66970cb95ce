// seat_kernels.hip -- greedy_seat_kernel, seat_rows_kernel and their launch functions (seat_rows.hpp describes them), as a translation unit of its own: its
// kernel-resource remarks are kept apart from the other units' (mate_amd/build.py: lib/kernel_resources_seat.json).
#include <hip/hip_runtime.h>
#include "seat_rows.hpp"

namespace mate {

// `sa` as it lies in the kernel-argument segment (fourth argument: behind the 8-byte `pp`, `g` and `q`)
__device__ __forceinline__ const SeatArgs &kernarg_seat_args(const SeatArgs &sa) {
    static_assert(alignof(SeatArgs) == 8 && sizeof(Ptrs) % 8 == 0 && sizeof(PolicyPtrs) % 8 == 0, "sa follows pp, g and q in the kernel arguments");
#if defined(__HIP_DEVICE_COMPILE__)
    (void)sa;
    return *(const SeatArgs *)((const char *)__builtin_amdgcn_kernarg_segment_ptr() + 8 + sizeof(Ptrs) + sizeof(PolicyPtrs));
#else
    return sa;
#endif
}

// The stand-alone agents' launch (greedy_policy_kernel: same records, same LDS slice, same lanes) on the generic shape, with one slot of the seat team
// left to the learner: its lane writes the learner's action into the joint row where the others write their agent's.
template <typename ObsT>
__global__ __launch_bounds__(256) void greedy_seat_kernel(const Params *__restrict__ pp, const Ptrs g_arg, const PolicyPtrs q_arg, const SeatArgs sa_arg) {
    // The argument records where they lie in the kernel-argument segment, read where they are used, the agents' and the seat's through pointers the
    // compiler takes for per-lane ones (greedy_channel_kernel: the generic-shape agents alone overflow the scalar registers when the records are preloaded).
    // Every lane reads the same address; a branch on such a field is the same in every lane.
    const Ptrs &g = kernarg_ptrs(g_arg);
    const PolicyPtrs *qv = &kernarg_policy_ptrs(q_arg);
    const SeatArgs *sv = &kernarg_seat_args(sa_arg);
    asm volatile("" : "+v"(qv));
    asm volatile("" : "+v"(sv));
    const PolicyPtrs &q = *qv;
    const SeatArgs &sa = *sv;
    const Params &p = *pp;
    extern __shared__ __align__(16) unsigned char seat_smem[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    // the four waves of a workgroup never synchronise: each owns one environment
    const int64_t env = (int64_t)blockIdx.x * 4 + wave;
    if (env >= g.N) return;
    unsigned char *base = seat_smem + wave * q.lds_bytes;
    // LDS: [policy record + staging][static record][dynamic record][mask words + one of slack]
    PolCtx<ObsT> a(p, q, base);
    double *st = reinterpret_cast<double *>(base + (size_t)(q.PW + policy_staging_words(p.Nc, p.Nt)) * 8);
    double *dy = st + p.SW;
    int32_t *di = reinterpret_cast<int32_t *>(dy + p.DF);
    uint32_t *mk = reinterpret_cast<uint32_t *>(dy + p.DW);
    {
        const double *src = q.pol + env * q.PW;
        for (int k = lane; k < q.PW; k += 64) a.f[k] = src[k];
        const double *s = g.stat + env * p.SW;
        for (int k = lane; k < p.SW; k += 64) st[k] = s[k];
        const double *d = g.dyn + env * p.DW;
        for (int k = lane; k < p.DW; k += 64) dy[k] = d[k];
        const uint32_t *m = q.masks + env * p.MW;
        for (int k = lane; k < p.MW; k += 64) mk[k] = m[k];
    }
    wave_sync();
    const int32_t *env_i = di + p.Nt * TI_STRIDE;
    if (g.freeze_done && env_i[EI_DONE] != 0) {                // finished, waiting for the batched reset: memory, actions and seat_acted stay
        if (lane == 0) sa.live[env] = 0;
        return;
    }
    const int z = seat_of_episode(p, sa.spec, env, env_i[EI_EPISODE]);
    const LiveSeat seat{p, g, q, sa.spec.team, z, env};
    greedy_policy_body<ObsT, 64, NoChannel, LiveSeat>(p, q, a, st, dy, di, mk, wave, lane, env, true, nullptr, nullptr, nullptr, nullptr, true, NoChannel(), seat);
    wave_sync();
    double *dst = q.pol + env * q.PW;
    for (int k = lane; k < q.PW; k += 64) dst[k] = a.f[k];
    if (lane == 0) { sa.acted[env] = z; sa.live[env] = 1; }
}

// A workgroup per tile of kSeatRowsEnvs environments: the seat's row of each into seat_obs, the seat into seat_index.
template <typename ObsT>
__global__ __launch_bounds__(256) void seat_rows_kernel(const Params *__restrict__ pp, const Ptrs g, const SeatRowsArgs a) {
    const Params &p = *pp;
    __shared__ int32_t seat_of[kSeatRowsEnvs];                 // the environment's seat, -1: the environment keeps its row
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * kSeatRowsEnvs;
    const int ne = (int)((g.N - e0) < (int64_t)kSeatRowsEnvs ? (g.N - e0) : (int64_t)kSeatRowsEnvs);
    if (tid < ne) {
        const int64_t env = e0 + tid;
        const int32_t *env_i = reinterpret_cast<const int32_t *>(g.dyn + env * p.DW + p.DF) + p.Nt * TI_STRIDE;
        const bool keep = a.live && a.live[env] == 0 && env_i[EI_DONE] != 0;      // idled through the whole call
        int z = -1;
        if (!keep) { z = seat_of_episode(p, a.spec, env, env_i[EI_EPISODE]); a.seat_index[env] = z; }
        seat_of[tid] = z;
    }
    __syncthreads();
    const int D = a.D, n = a.spec.n;
    const ObsT *src = reinterpret_cast<const ObsT *>(a.rows) + e0 * n * D;
    ObsT *dst = reinterpret_cast<ObsT *>(a.seat_obs) + e0 * D;      // (16-byte aligned: e0 D elements is a multiple of 16 D)
    constexpr int W = 16 / (int)sizeof(ObsT);
    typedef ObsT vec_t __attribute__((ext_vector_type(W)));
    const int total = ne * D;
    for (int v = tid; v * W < total; v += 256) {
        const int x0 = v * W;
        vec_t out;
        bool whole = x0 + W <= total;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const int x = x0 + k;
            ObsT value = (ObsT)0;
            if (x < total) {
                const int e = x / D, col = x - e * D, z = seat_of[e];
                if (z >= 0) value = src[((int64_t)e * n + z) * D + col];
                else whole = false;
            }
            out[k] = value;
        }
        if (whole) reinterpret_cast<vec_t *>(dst)[v] = out;
        else {
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const int x = x0 + k;
                if (x < total && seat_of[x / D] >= 0) dst[x] = out[k];
            }
        }
    }
}

hipError_t launch_greedy_seat(bool obs_f64, unsigned blocks, size_t lds, hipStream_t stream, const Params *params, const Ptrs &g, const PolicyPtrs &q, const SeatArgs &a) {
    if (obs_f64) hipLaunchKernelGGL(greedy_seat_kernel<double>, dim3(blocks), dim3(256), lds, stream, params, g, q, a);
    else hipLaunchKernelGGL(greedy_seat_kernel<float>, dim3(blocks), dim3(256), lds, stream, params, g, q, a);
    return hipGetLastError();
}

const void *greedy_seat_function(bool obs_f64) {
    return obs_f64 ? reinterpret_cast<const void *>(greedy_seat_kernel<double>) : reinterpret_cast<const void *>(greedy_seat_kernel<float>);
}

hipError_t launch_seat_rows(bool obs_f64, unsigned blocks, hipStream_t stream, const Params *params, const Ptrs &g, const SeatRowsArgs &a) {
    if (obs_f64) hipLaunchKernelGGL(seat_rows_kernel<double>, dim3(blocks), dim3(256), 0, stream, params, g, a);
    else hipLaunchKernelGGL(seat_rows_kernel<float>, dim3(blocks), dim3(256), 0, stream, params, g, a);
    return hipGetLastError();
}

}  // namespace mate
