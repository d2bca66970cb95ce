// channel_kernels.hip -- greedy_channel_kernel and its launch function (channel_rows.hpp describes them), as a translation unit of its own: its
// kernel-resource remarks are kept apart from the other units' (mate_amd/build.py: lib/kernel_resources_channel.json).
#include <hip/hip_runtime.h>
#include "channel_rows.hpp"

namespace mate {

// `ca` as it lies in the kernel-argument segment (fourth argument: behind the 8-byte `pp`, `g` and `q`)
__device__ __forceinline__ const ChannelArgs &kernarg_channel_args(const ChannelArgs &ca) {
    static_assert(alignof(ChannelArgs) == 8 && sizeof(Ptrs) % 8 == 0 && sizeof(PolicyPtrs) % 8 == 0, "ca follows pp, g and q in the kernel arguments");
#if defined(__HIP_DEVICE_COMPILE__)
    (void)ca;
    return *(const ChannelArgs *)((const char *)__builtin_amdgcn_kernarg_segment_ptr() + 8 + sizeof(Ptrs) + sizeof(PolicyPtrs));
#else
    return ca;
#endif
}

// The stand-alone agents' launch (greedy_policy_kernel: same records, same LDS slice, same lanes) on the generic shape, with the channel inside
// the agents' `communicate` phase and the two edge matrices of every acting team behind it.
template <typename ObsT>
__global__ __launch_bounds__(256) void greedy_channel_kernel(const Params *__restrict__ pp, const Ptrs g_arg, const PolicyPtrs q_arg, const ChannelArgs ca_arg) {
    // The three argument records where they lie in the kernel-argument segment, read where they are used (kernarg_ptrs, kernarg_policy_ptrs): preloaded
    // into scalar registers at entry and kept for the whole kernel they spilled 66 of them into vector lanes.  The agents' and the channel's records are
    // read through pointers the compiler takes for per-lane ones: their fields (the seven tape pointers, the channel's settings and buffers of both
    // teams) then live in vector registers, of which the kernel has plenty, not in the 102 scalar ones the generic-shape agents alone overflow (the
    // stand-alone greedy_policy_kernel<AnyShape> spills 29).  Every lane reads the same address; a branch on such a field is the same in every lane.
    // (Copying the agents' record whole at entry and reading the channel's common fields there -- one round trip for all of them -- measured SLOWER:
    // 8.77 against 8.40 us per launch at 4096 x MATE-4v8-9, 114 VGPRs against 76.)
    const Ptrs &g = kernarg_ptrs(g_arg);
    const PolicyPtrs *qv = &kernarg_policy_ptrs(q_arg);
    const ChannelArgs *cv = &kernarg_channel_args(ca_arg);
    asm volatile("" : "+v"(qv));
    asm volatile("" : "+v"(cv));
    const PolicyPtrs &q = *qv;
    const ChannelArgs &ca = *cv;
    const Params &p = *pp;
    extern __shared__ __align__(16) unsigned char channel_smem[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    // the four waves of a workgroup never synchronise: each owns one environment
    const int64_t env = (int64_t)blockIdx.x * 4 + wave;
    if (env >= g.N) return;
    unsigned char *base = channel_smem + wave * ca.lds_bytes;
    // LDS: [policy record + staging][static record][dynamic record][mask words + one of slack][edge staging]
    PolCtx<ObsT> a(p, q, base);
    double *st = reinterpret_cast<double *>(base + (size_t)(q.PW + policy_staging_words(p.Nc, p.Nt)) * 8);
    double *dy = st + p.SW;
    int32_t *di = reinterpret_cast<int32_t *>(dy + p.DF);
    uint32_t *mk = reinterpret_cast<uint32_t *>(dy + p.DW);
    int8_t *stage = reinterpret_cast<int8_t *>(base + q.lds_bytes);      // (16-byte aligned: both byte counts are multiples of 16)
    const int Nc = p.Nc, Nt = p.Nt;
    const int cam_bytes = channel_matrix_bytes(Nc), tgt_bytes = channel_matrix_bytes(Nt);
    {
        const double *src = q.pol + env * q.PW;
        for (int k = lane; k < q.PW; k += 64) a.f[k] = src[k];
        const double *s = g.stat + env * p.SW;
        for (int k = lane; k < p.SW; k += 64) st[k] = s[k];
        const double *d = g.dyn + env * p.DW;
        for (int k = lane; k < p.DW; k += 64) dy[k] = d[k];
        const uint32_t *m = q.masks + env * p.MW;
        for (int k = lane; k < p.MW; k += 64) mk[k] = m[k];
        int32_t *z = reinterpret_cast<int32_t *>(stage);
        for (int k = lane; k < (cam_bytes + tgt_bytes) / 2; k += 64) z[k] = 0;
    }
    wave_sync();
    const int32_t *env_i = di + Nt * TI_STRIDE;
    if (g.freeze_done && env_i[EI_DONE] != 0) return;          // finished, waiting for the batched reset: memory, actions and edge rows stay
    const bool cams = q.caller_team != 0, tgts = q.caller_team != 1;
    bool talk_c = cams, talk_t = tgts;
    if (cams && ca.team[0].mix.on) talk_c = channel_mixture_kind(p, ca.team[0].mix, 0, env, env_i[EI_EPISODE]) == SCRIPTED_GREEDY;
    if (tgts && ca.team[1].mix.on) { const int kind = channel_mixture_kind(p, ca.team[1].mix, 1, env, env_i[EI_EPISODE]); talk_t = kind == SCRIPTED_GREEDY || kind == SCRIPTED_HEURISTIC; }
    const LiveChannel ch{p, ca, st, dy, stage, env, p.first_env + (uint32_t)env, (uint32_t)env_i[EI_TICK], talk_c, talk_t};
    greedy_policy_body<ObsT, 64, LiveChannel>(p, q, a, st, dy, di, mk, wave, lane, env, true, nullptr, nullptr, nullptr, nullptr, true, ch);
    wave_sync();
    double *dst = q.pol + env * q.PW;
    for (int k = lane; k < q.PW; k += 64) dst[k] = a.f[k];
    // the edge matrices of the teams that acted: whole 4-byte words where the matrix is a whole number of them, bytes else
    for (int team = 0; team < 2; ++team) {
        if (team == 0 ? !cams : !tgts) continue;
        const ChannelTeam &T = ca.team[team];
        const int n = team == 0 ? Nc : Nt, nb = n * n, padded = team == 0 ? cam_bytes : tgt_bytes;
        const int8_t *src = stage + (team == 0 ? 0 : 2 * cam_bytes);
        int8_t *sent = T.sent + env * nb, *delivered = T.delivered + env * nb;
        if ((nb & 3) == 0) {
            for (int k = lane; k < nb / 4; k += 64) {
                reinterpret_cast<int32_t *>(sent)[k] = reinterpret_cast<const int32_t *>(src)[k];
                reinterpret_cast<int32_t *>(delivered)[k] = reinterpret_cast<const int32_t *>(src + padded)[k];
            }
        } else {
            for (int k = lane; k < nb; k += 64) { sent[k] = src[k]; delivered[k] = src[padded + k]; }
        }
    }
    // a team that did not act drew nothing
    if (!cams && ca.team[0].record_u) for (int k = lane; k < Nc * Nc; k += 64) ca.team[0].record_u[env * (Nc * Nc) + k] = __builtin_nan("");
    if (!tgts && ca.team[1].record_u) for (int k = lane; k < Nt * Nt; k += 64) ca.team[1].record_u[env * (Nt * Nt) + k] = __builtin_nan("");
}

hipError_t launch_greedy_channel(bool obs_f64, unsigned blocks, size_t lds, hipStream_t stream, const Params *params, const Ptrs &g, const PolicyPtrs &q, const ChannelArgs &a) {
    if (obs_f64) hipLaunchKernelGGL(greedy_channel_kernel<double>, dim3(blocks), dim3(256), lds, stream, params, g, q, a);
    else hipLaunchKernelGGL(greedy_channel_kernel<float>, dim3(blocks), dim3(256), lds, stream, params, g, q, a);
    return hipGetLastError();
}

const void *greedy_channel_function(bool obs_f64) {
    return obs_f64 ? reinterpret_cast<const void *>(greedy_channel_kernel<double>) : reinterpret_cast<const void *>(greedy_channel_kernel<float>);
}

}  // namespace mate
