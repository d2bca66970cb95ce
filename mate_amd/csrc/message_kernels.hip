// message_kernels.hip -- message_rows_kernel and its launch function (message_rows.hpp describes them), as a translation unit of its own: its
// kernel-resource remarks are kept apart from the other units' (mate_amd/build.py: lib/kernel_resources_message.json).
#include <hip/hip_runtime.h>
#include "message_rows.hpp"

namespace mate {

// `a` as it lies in the kernel-argument segment (third argument: behind the 8-byte `pp` and `g`)
__device__ __forceinline__ const MessageArgs &kernarg_message_args(const MessageArgs &a) {
    static_assert(alignof(MessageArgs) == 8 && sizeof(Ptrs) % 8 == 0, "a follows pp and g in the kernel arguments");
#if defined(__HIP_DEVICE_COMPILE__)
    (void)a;
    return *(const MessageArgs *)((const char *)__builtin_amdgcn_kernarg_segment_ptr() + 8 + sizeof(Ptrs));
#else
    return a;
#endif
}

// One wave per environment, four per workgroup; both teams one after the other.  Per team: the verdicts (a pair per lane, 64 per round), the counts under
// the tag rule, the edge matrices, the two sums per agent, then the inbox block as one contiguous stream.
template <typename ObsT>
__global__ __launch_bounds__(256) void message_rows_kernel(const Params *__restrict__ pp, const Ptrs g_arg, const MessageArgs a_arg) {
    // the argument records where they lie in the kernel-argument segment, read where they are used (every field is the same in every lane)
    const Ptrs &g = kernarg_ptrs(g_arg);
    const MessageArgs &a = kernarg_message_args(a_arg);
    const Params &p = *pp;
    __shared__ uint64_t words_s[4][kMessagePairs / 64];                     // delivered, bit s n + r
    __shared__ __align__(4) int8_t stage_s[4][2 * kMessagePairs];           // [sent | delivered] of the call
    __shared__ int32_t count_s[4][kMessagePairs];                           // step_edges as stored
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    // the four waves of a workgroup never synchronise: each owns one environment
    const int64_t env = (int64_t)blockIdx.x * 4 + wave;
    if (env >= g.N) return;
    const int32_t *env_i = reinterpret_cast<const int32_t *>(g.dyn + env * p.DW + p.DF) + p.Nt * TI_STRIDE;
    if (env_i[EI_DONE] != 0) return;                           // the episode is over: every row stays
    const int32_t tick = env_i[EI_TICK], episode = env_i[EI_EPISODE];
    uint64_t *words = words_s[wave];
    int8_t *stage = stage_s[wave];
    int32_t *count = count_s[wave];
    for (int team = 0; team < 2; ++team) {
        const MessageTeam &T = a.team[team];
        if (!T.on) continue;
        const int n = T.n, nn = n * n;
        // the positions the team's observation rows show: the static record's for cameras, the dynamic record's for targets; x[n] then y[n] in either
        const double *xs = team == 0 ? g.stat + env * p.SW : g.dyn + env * p.DW + 2 * p.Nc, *ys = xs + n;
        int32_t *tags = T.tags + env * 2;
        const int32_t tag_tick = tags[0], tag_episode = tags[1];
        const bool new_episode = tag_episode != episode, new_tick = new_episode || tag_tick != tick;
        const int64_t e0 = env * nn;
        for (int base = 0; base < nn; base += 64) {
            const int k = base + lane;
            bool got = false;
            if (k < nn) {
                const int s = k / n, r = k - s * n;
                const bool sent = T.address ? T.address[e0 + k] != 0 : true;
                double u_used = __builtin_nan("");
                if (sent) {
                    got = true;
                    if (T.set) {
                        double u = 0.0, dist = 0.0;
                        int mask = 1;
                        if (T.rate > 0.0) {
                            if (T.tape_u) u = T.tape_u[e0 + k];
                            else u = (double)philox(p.seed_lo, p.seed_hi, p.first_env + (uint32_t)env, (uint32_t)tick, S_MSG_DROP, message_draw_key(a.round, team, s, r)).x * 2.3283064365386963e-10;
                            u_used = u;
                        }
                        if (T.limit >= 0.0) dist = norm2(xs[r] - xs[s], ys[r] - ys[s]);
                        if (T.mask) mask = T.mask[e0 + k];
                        got = channel_verdict(T.disabled != 0, T.limit, T.rate, mask, u, dist);
                    }
                }
                if (T.record_u) T.record_u[e0 + k] = u_used;
                int32_t step = T.step_edges[e0 + k], total = T.total_edges[e0 + k];
                if (new_episode) step = total = 0;
                else if (new_tick) { total += step; step = 0; }
                step += got ? 1 : 0;
                T.step_edges[e0 + k] = step; T.total_edges[e0 + k] = total;
                stage[k] = sent ? 1 : 0; stage[kMessagePairs + k] = got ? 1 : 0; count[k] = step;
            }
            const uint64_t word = __ballot(got);
            if (lane == 0) words[base >> 6] = word;
        }
        wave_sync();
        if (lane == 0 && new_tick) { tags[0] = tick; tags[1] = episode; }
        // the edge matrices of the call: whole 4-byte words where the matrix is a whole number of them, bytes else
        {
            int8_t *sent = T.sent + e0, *delivered = T.delivered + e0;
            if ((nn & 3) == 0) {
                for (int k = lane; k < nn / 4; k += 64) {
                    reinterpret_cast<int32_t *>(sent)[k] = reinterpret_cast<const int32_t *>(stage)[k];
                    reinterpret_cast<int32_t *>(delivered)[k] = reinterpret_cast<const int32_t *>(stage + kMessagePairs)[k];
                }
            } else {
                for (int k = lane; k < nn; k += 64) { sent[k] = stage[k]; delivered[k] = stage[kMessagePairs + k]; }
            }
        }
        // out_ / in_communication_edges of agent `lane`: the row and the column sum of step_edges
        if (lane < n) {
            int32_t out = 0, in = 0;
            for (int j = 0; j < n; ++j) { out += count[lane * n + j]; in += count[j * n + lane]; }
            int32_t *dst = T.agent_edges + (env * n + lane) * 2;
            dst[0] = out; dst[1] = in;
        }
        // the inbox block [recipient][sender][width], one contiguous stream: the sender's content where its bit is set, zeros else
        const int M = T.width, row_bytes = M * (int)sizeof(ObsT);
        const int64_t rows_in = env * (T.pairwise ? nn : n);
        if ((row_bytes & 15) == 0) {
            typedef uint32_t chunk_t __attribute__((ext_vector_type(4)));
            const int C = row_bytes >> 4, per_recipient = n * C, total = n * per_recipient;
            const chunk_t *src = reinterpret_cast<const chunk_t *>(T.payload) + rows_in * C;
            chunk_t *dst = reinterpret_cast<chunk_t *>(T.inbox) + e0 * C;
            // four chunks per lane and pass, the loads of all four ahead of the stores: one round trip per pass instead of one per chunk
            for (int j0 = lane; j0 < total; j0 += 256) {
                chunk_t v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = j0 + 64 * q;
                    v[q] = chunk_t{0u, 0u, 0u, 0u};
                    if (j < total) {
                        const int r = j / per_recipient, rest = j - r * per_recipient, s = rest / C, c = rest - s * C, k = s * n + r;
                        if ((words[k >> 6] >> (k & 63)) & 1ull) v[q] = src[(T.pairwise ? k : s) * C + c];
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = j0 + 64 * q;
                    if (j < total) __builtin_nontemporal_store(v[q], dst + j);
                }
            }
        } else {
            const int per_recipient = n * M, total = n * per_recipient;
            const ObsT *src = reinterpret_cast<const ObsT *>(T.payload) + rows_in * M;
            ObsT *dst = reinterpret_cast<ObsT *>(T.inbox) + e0 * M;
            for (int j = lane; j < total; j += 64) {
                const int r = j / per_recipient, rest = j - r * per_recipient, s = rest / M, c = rest - s * M, k = s * n + r;
                ObsT v = (ObsT)0;
                if ((words[k >> 6] >> (k & 63)) & 1ull) v = src[(T.pairwise ? k : s) * M + c];
                dst[j] = v;
            }
        }
        wave_sync();                                           // (the next team stages into the same LDS)
    }
}

hipError_t launch_message_rows(bool obs_f64, unsigned blocks, hipStream_t stream, const Params *params, const Ptrs &g, const MessageArgs &a) {
    if (obs_f64) hipLaunchKernelGGL(message_rows_kernel<double>, dim3(blocks), dim3(256), 0, stream, params, g, a);
    else hipLaunchKernelGGL(message_rows_kernel<float>, dim3(blocks), dim3(256), 0, stream, params, g, a);
    return hipGetLastError();
}

}  // namespace mate
