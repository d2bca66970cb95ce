// episode_kernels.hip -- episode_rows_kernel and its launch function (episode_rows.hpp describes them), as a translation unit of its own: its
// kernel-resource remarks are kept apart from the other units' (mate_amd/build.py: lib/kernel_resources_episodes.json).
#include <hip/hip_runtime.h>
#include "episode_rows.hpp"

namespace mate {

__device__ __forceinline__ int episode_group_sum(int v) {
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 16);
    return v;
}
// the sum over agents 0 .. A - 1 of a row held one element per lane of the group, in agent order (every lane of the group ends with it)
__device__ __forceinline__ double episode_row_sum(double mine, int A) {
    double s = 0.0;
    for (int k = 0; k < A; ++k) s = s + __shfl(mine, k, 16);
    return s;
}
// the team reward once per agent, summed the same way
__device__ __forceinline__ double episode_repeated_sum(double r, int A) {
    double s = 0.0;
    for (int k = 0; k < A; ++k) s = s + r;
    return s;
}

struct EpisodeTile { bool finishing; double column; };      // the group's environment ends an episode in this launch; lane j's column of its record

// One tile: the sums of its sixteen environments through this call's learner steps.  Called by every thread of the workgroup (the shuffles want whole groups).
__device__ __forceinline__ EpisodeTile episode_tile(const Params &p, const EpisodeArgs &a, int64_t e0, int tid) {
    const int Nc = p.Nc, Nt = p.Nt;
    const int el = tid >> 4, j = tid & 15;
    const int64_t env = e0 + el;
    const bool present = env < a.N;
    const bool camera = a.team == 0;
    const bool want_tracked = camera && a.masks != nullptr;
    const ViewWords vw = view_words(a.bit_ct, Nc, Nt);
    uint32_t word_mask = 0u;                                     // the view bits inside lane j's word
    if (j < vw.count) {
        const int lo = j == 0 ? vw.origin : 0, hi = vw.origin + Nc * Nt - 32 * j;
        word_mask = (hi >= 32 ? 0xffffffffu : (1u << hi) - 1u) & ~((1u << lo) - 1u);
    }

    double mine = 0.0;
    int32_t episode_word = 0, length = 0;
    if (present) {
        if (j < kEpisodeWords) mine = a.sums[env * kEpisodeWords + j];
        const int32_t *ei = reinterpret_cast<const int32_t *>(a.dyn + env * p.DW + p.DF) + Nt * TI_STRIDE;
        episode_word = ei[EI_EPISODE]; length = ei[EI_EPSTEP];
    }
    const double episode = (double)(uint32_t)episode_word;
    const bool kept = __shfl(mine, EW_TAG, 16) == episode;       // (NaN, the cleared tag: never)
    double steps = __shfl(mine, EW_STEPS, 16), frames = __shfl(mine, EW_FRAMES, 16), raw = __shfl(mine, EW_RAW, 16), norm = __shfl(mine, EW_NORM, 16),
           reward = __shfl(mine, EW_REWARD, 16), coverage = __shfl(mine, EW_COVERAGE, 16), real = __shfl(mine, EW_REAL, 16), tracked = __shfl(mine, EW_TRACKED, 16);
    if (!kept) { steps = 0.0; frames = 0.0; raw = 0.0; norm = 0.0; reward = 0.0; coverage = 0.0; real = 0.0; tracked = 0.0; }

    // the learner's reward row of this step where one exists: the attached reward rows (a one-frame call)
    double row_element = 0.0;
    if (a.rows && present && j < a.A) row_element = a.rows_f64 ? reinterpret_cast<const double *>(a.rows)[env * a.A + j] : (double)reinterpret_cast<const float *>(a.rows)[env * a.A + j];
    const double row_sum = episode_row_sum(row_element, a.A);

    bool finished = false;
    double last_mtr = 0.0, last_cargo = 0.0;
    for (int f = 0; f < a.K; ++f) {
        float4 lo = make_float4(0.f, 0.f, 2.f, 0.f), hi = make_float4(0.f, 0.f, 0.f, 0.f);
        if (present) {
            const float4 *rec = reinterpret_cast<const float4 *>(a.scalars + ((int64_t)f * a.N + env) * 8);
            lo = rec[0]; hi = rec[1];
        }
        const bool live = lo.z != 2.0f && !finished;             // (the same in all sixteen lanes of the group)
        int seen = 0;
        if (want_tracked) {
            uint32_t w = 0u;
            if (live && j < vw.count) w = a.masks[((int64_t)f * a.N + env) * p.MW + vw.first + j] & word_mask;
            seen = episode_group_sum(__popc(w));
        }
        if (live) {
            const double step_tracked = want_tracked ? (double)seen / (double)Nc : NAN;
            const double r = camera ? (double)lo.x : (double)lo.y, nr = camera ? -(double)hi.w : (double)hi.w;
            steps = steps + 1.0; frames = frames + 1.0;
            raw = raw + r; norm = norm + nr;
            reward = reward + (a.reward_nan ? NAN : a.rows ? row_sum : episode_repeated_sum(r, a.A));
            coverage = coverage + (double)lo.w; real = real + (double)hi.x;
            last_mtr = (double)hi.y; last_cargo = (double)hi.z;
            tracked = tracked + step_tracked;
            finished = lo.z == 1.0f;
        }
    }

    EpisodeTile out;
    out.finishing = present && finished;
    const double columns[kEpisodeColumns] = {(double)((int64_t)p.first_env + env), episode, steps, frames, (double)length, raw, norm, reward,
                                             raw / steps, norm / steps, coverage / steps, real / steps, last_mtr, last_cargo, tracked / steps, (double)a.team};
    out.column = columns[0];
#pragma unroll
    for (int k = 1; k < kEpisodeColumns; ++k) out.column = j == k ? columns[k] : out.column;
    // the sums the next launch continues from: cleared behind a record
    const double words[kEpisodeWords] = {finished ? NAN : episode, finished ? 0.0 : steps, finished ? 0.0 : frames, finished ? 0.0 : raw, finished ? 0.0 : norm,
                                         finished ? 0.0 : reward, finished ? 0.0 : coverage, finished ? 0.0 : real, finished ? 0.0 : tracked};
    double word = words[0];
#pragma unroll
    for (int k = 1; k < kEpisodeWords; ++k) word = j == k ? words[k] : word;
    if (present && j < kEpisodeWords) a.sums[env * kEpisodeWords + j] = word;
    return out;
}

// The launch arguments are read from the kernel-argument segment where they are used (kernarg_ptrs' way, engine_kernels.hpp): preloaded at entry and kept for the whole
// kernel, the pointers and the scenario constants were more scalar registers than a wave has.
__device__ __forceinline__ const EpisodeArgs &kernarg_episode_args(const EpisodeArgs &a) {
    static_assert(alignof(EpisodeArgs) == 8 && sizeof(const Params *) == 8, "a follows pp at byte 8 of the kernel arguments");
#if defined(__HIP_DEVICE_COMPILE__)
    (void)a;
    return *(const EpisodeArgs *)((const char *)__builtin_amdgcn_kernarg_segment_ptr() + 8);
#else
    return a;
#endif
}

__global__ __launch_bounds__(256) void episode_rows_kernel(const Params *__restrict__ pp, const EpisodeArgs a_) {
    __shared__ unsigned long long serial_count;
    const Params &p = *pp;
    const EpisodeArgs &a = kernarg_episode_args(a_);
    const int tid = threadIdx.x, el = tid >> 4, j = tid & 15, lane = tid & 63;
    // a workgroup per tile -- or the serial form (capacity < N): ONE workgroup, the tiles one after the other, a group at a time between barriers, so that a
    // later record overwrites an earlier one's slot
    const int64_t first = a.serial ? 0 : (int64_t)blockIdx.x * kAttachedEnvsPerBlock, end = a.serial ? a.N : first + 1;
    if (a.serial) {
        if (tid == 0) serial_count = *a.count;
        __syncthreads();
    }
    for (int64_t e0 = first; e0 < end; e0 += kAttachedEnvsPerBlock) {
        const EpisodeTile t = episode_tile(p, a, e0, tid);
        if (!a.serial) {
            // one atomic add per wave: the groups that finish take consecutive record numbers
            const unsigned long long ballot = __ballot(t.finishing && j == 0);
            if (ballot != 0ull) {                                // (wave-uniform)
                const int leader = __ffsll((unsigned long long)ballot) - 1;
                unsigned long long base = 0ull;
                if (lane == leader) base = atomicAdd(a.count, (unsigned long long)__popcll(ballot));
                base = __shfl(base, leader, 64);
                const int rank = __popcll(ballot & ((1ull << (lane & ~15)) - 1ull));
                if (t.finishing) a.records[((base + (unsigned long long)rank) % (unsigned long long)a.capacity) * kEpisodeColumns + j] = t.column;
            }
        } else {
            for (int g = 0; g < kAttachedEnvsPerBlock; ++g) {
                unsigned long long n = 0ull;
                if (el == g && j == 0) n = serial_count;
                n = __shfl(n, 0, 16);
                if (el == g && t.finishing) {
                    a.records[(n % (unsigned long long)a.capacity) * kEpisodeColumns + j] = t.column;
                    if (j == 0) serial_count = n + 1ull;
                }
                __syncthreads();
            }
        }
    }
    if (a.serial && tid == 0) *a.count = serial_count;
}

hipError_t launch_episode_rows(unsigned blocks, hipStream_t stream, const Params *params, const EpisodeArgs &a) {
    hipLaunchKernelGGL(episode_rows_kernel, dim3(blocks), dim3(256), 0, stream, params, a);
    return hipGetLastError();
}

}  // namespace mate
