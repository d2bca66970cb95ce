// scripted_kernels.hip -- scripted_opponent_kernel and its launch function (scripted_rows.hpp describes them), as a translation unit of its own: its
// kernel-resource remarks are kept apart from the other units' (mate_amd/build.py: lib/kernel_resources_scripted.json).
#include <hip/hip_runtime.h>
#include "scripted_rows.hpp"

namespace mate {

constexpr double kU32 = 2.3283064365386963e-10;      // 2^-32: a 32-bit word as a uniform in [0, 1), as the Greedy agents' draws

// The mixture draw: the first candidate with u < cum (searchsorted side='right'), the last where rounding leaves cum[count - 1] short of u.
// (Constant indices only: the arguments stay in scalar registers, nothing is copied to private memory.)
__device__ __forceinline__ int scripted_pick(const ScriptedTeam &T, double u) {
    int kind = -1;
#pragma unroll
    for (int i = kScriptedKinds - 1; i >= 0; --i)
        if (i < T.count && (u < T.cum[i] || i == T.count - 1)) kind = T.kinds[i];
    return kind;
}
__device__ __forceinline__ bool scripted_member(const ScriptedTeam &T, int kind) {
    bool member = false;
#pragma unroll
    for (int i = 0; i < kScriptedKinds; ++i) member |= i < T.count && T.kinds[i] == kind;
    return member;
}

// One team of one environment; lane j < T.n is agent j.  `frozen`: the agents' launch skipped the environment.
template <int TEAM>
__device__ __forceinline__ void scripted_team(const Params &p, const ScriptedArgs &a, int64_t N, const double *d, const int32_t *di, int64_t env, int j, bool frozen, uint64_t capword) {
    const ScriptedTeam &T = a.team[TEAM];
    if (!T.on) return;                                   // (the same in every lane of the launch)
    const int Nc = p.Nc, Nt = p.Nt, n = T.n;
    const bool agent = j < n;
    const int64_t o = env * n + j;
    const int32_t *env_i = di + Nt * TI_STRIDE;
    const double nan = __builtin_nan("");
    double rec[4] = {nan, nan, nan, nan}, rec_reset[4] = {nan, nan, nan, nan};      // (constant indices: registers)
    int kind = T.choice[env];
    if (!frozen) {
        const int32_t episode = env_i[EI_EPISODE];
        const uint32_t tick = (uint32_t)env_i[EI_TICK], env_global = p.first_env + (uint32_t)env;
        const bool fresh = T.episode[env] != episode;   // the team's first acting call of the episode: the mixture's reset
        int counter = fresh ? 0 : T.counter[env];
        if (fresh) {
            const int taped = a.tape.choice ? a.tape.choice[(int64_t)TEAM * N + env] : -1;
            if (scripted_member(T, taped)) kind = taped;
            else { const U4 r = philox(p.seed_lo, p.seed_hi, env_global, (uint32_t)episode, S_SCR_CHOICE, (uint32_t)TEAM); kind = scripted_pick(T, u53(r.x, r.y)); }
        }
        const bool sample_now = counter % T.frame_skip == 0;     // RandomAgent: episode_step % frame_skip == 0 (random.py:52, :102)
        if (agent) {
            double ax = 0.0, ay = 0.0;
            if (kind == SCRIPTED_NAIVE || kind == SCRIPTED_RANDOM) {
                if (TEAM == SCRIPTED_CAMERAS) {
                    double u0, u1;
                    if (a.tape.camera_u) { u0 = a.tape.camera_u[o * 2]; u1 = a.tape.camera_u[o * 2 + 1]; }
                    else { const U4 r = philox(p.seed_lo, p.seed_hi, env_global, tick, S_SCR_CAMERA, (uint32_t)j); u0 = (double)r.x * kU32; u1 = (double)r.y * kU32; }
                    if (kind == SCRIPTED_NAIVE) {                // np_random.uniform(0.0, 0.4) * action_space.high (naive.py:27)
                        const double m = 0.0 + 0.4 * u0;
                        ax = m * p.rot; ay = m * p.zoom;
                        rec[0] = u0;
                    } else if (sample_now) {                     // action_space.sample()
                        ax = -p.rot + (2.0 * p.rot) * u0; ay = -p.zoom + (2.0 * p.zoom) * u1;
                        rec[0] = u0; rec[1] = u1;
                    } else { const double2 v = reinterpret_cast<const double2 *>(T.prev_action)[o]; ax = v.x; ay = v.y; }
                } else {
                    const double step_size = ((capword >> j) & 1ull) ? p.tgt_step * 0.5 : p.tgt_step;
                    double ub, u0, u1;
                    if (a.tape.target_u) { ub = a.tape.target_u[o * 3]; u0 = a.tape.target_u[o * 3 + 1]; u1 = a.tape.target_u[o * 3 + 2]; }
                    else { const U4 r = philox(p.seed_lo, p.seed_hi, env_global, tick, S_SCR_TARGET, (uint32_t)j); ub = (double)r.x * kU32; u0 = (double)r.y * kU32; u1 = (double)r.z * kU32; }
                    if (kind == SCRIPTED_NAIVE) {
                        const double x = d[2 * Nc + j], y = d[2 * Nc + Nt + j];
                        const int gw = di[j * TI_STRIDE + TI_GW];
                        int goal, inc;
                        double plx, ply, nx, ny;
                        if (fresh) {                             // NaiveTargetAgent.reset (naive.py:56-68)
                            double r0, r1, rg, ri;
                            if (a.tape.target_reset) { r0 = a.tape.target_reset[o * 4]; r1 = a.tape.target_reset[o * 4 + 1]; rg = a.tape.target_reset[o * 4 + 2]; ri = a.tape.target_reset[o * 4 + 3]; }
                            else {
                                const U4 r = philox(p.seed_lo, p.seed_hi, env_global, (uint32_t)episode, S_SCR_TARGET_RESET, (uint32_t)j);
                                r0 = (double)r.x * kU32; r1 = (double)r.y * kU32; rg = (double)(r.z >> 30); ri = (r.w >> 31) ? -1.0 : 1.0;
                            }
                            nx = 0.5 * (-step_size + (2.0 * step_size) * r0); ny = 0.5 * (-step_size + (2.0 * step_size) * r1);
                            goal = (int)rg; goal = goal < 0 ? 0 : (goal > 3 ? 3 : goal);
                            inc = ri < 0.0 ? -1 : 1;
                            plx = x; ply = y;
                            rec_reset[0] = r0; rec_reset[1] = r1; rec_reset[2] = (double)goal; rec_reset[3] = (double)inc;
                        } else {
                            goal = T.goal[o]; inc = T.inc[o];
                            const double2 l = reinterpret_cast<const double2 *>(T.prev_location)[o], v = reinterpret_cast<const double2 *>(T.prev_noise)[o];
                            plx = l.x; ply = l.y; nx = v.x; ny = v.y;
                        }
                        {   // the arrival rule (naive.py:79-86)
                            const double wx = (goal == 0 || goal == 3) ? kWarehouseCenter : -kWarehouseCenter, wy = (goal < 2) ? kWarehouseCenter : -kWarehouseCenter;
                            if (norm2(x - wx, y - wy) <= 0.9 * kWarehouseRadius) {
                                const bool carries = (gw & 0xff) != 0 && ((gw >> 8) & 0xff) > 0;      // goal_bits.any()
                                const int empty = (gw >> 16) & 0xf;
                                goal = (goal + inc) & 3;
                                if (!carries && empty != 0xf)
                                    for (int s = 0; s < 3 && ((empty >> goal) & 1); ++s) goal = (goal + inc) & 3;
                            }
                        }
                        const double wx = (goal == 0 || goal == 3) ? kWarehouseCenter : -kWarehouseCenter, wy = (goal < 2) ? kWarehouseCenter : -kWarehouseCenter;
                        double gx = wx - x, gy = wy - y;
                        const double len = norm2(gx, gy);
                        if (len > step_size) { const double k2 = div_nz(step_size, len); gx *= k2; gy *= k2; }
                        // the noise rule of GreedyTargetAgent.act as greedy_policy_body has it (policy_kernels.hpp), noise_scale 0.5
                        const double prob = norm2(x - plx, y - ply) > 0.2 * step_size ? 0.05 : 0.75;
                        rec[0] = ub;
                        if ((prob <= 0.5) ? (ub > 1.0 - prob) : (ub <= prob)) {
                            nx = 0.5 * (-step_size + (2.0 * step_size) * u0); ny = 0.5 * (-step_size + (2.0 * step_size) * u1);
                            rec[1] = u0; rec[2] = u1;
                        }
                        ax = clipd(gx + nx, -step_size, step_size); ay = clipd(gy + ny, -step_size, step_size);
                        T.goal[o] = goal; T.inc[o] = inc;
                        reinterpret_cast<double2 *>(T.prev_location)[o] = make_double2(x, y);
                        reinterpret_cast<double2 *>(T.prev_noise)[o] = make_double2(nx, ny);
                    } else if (sample_now) {
                        ax = -step_size + (2.0 * step_size) * u0; ay = -step_size + (2.0 * step_size) * u1;
                        rec[1] = u0; rec[2] = u1;
                    } else { const double2 v = reinterpret_cast<const double2 *>(T.prev_action)[o]; ax = v.x; ay = v.y; }
                }
                if (kind == SCRIPTED_RANDOM && sample_now) reinterpret_cast<double2 *>(T.prev_action)[o] = make_double2(ax, ay);
            } else {                                             // another launch's row, or the caller's
                const double *src = kind == SCRIPTED_GREEDY ? T.rows[SCRIPTED_GREEDY] : (kind == SCRIPTED_HEURISTIC ? T.rows[SCRIPTED_HEURISTIC] : T.rows[SCRIPTED_EXTERNAL]);
                const double2 v = reinterpret_cast<const double2 *>(src)[o];
                ax = v.x; ay = v.y;
            }
            reinterpret_cast<double2 *>(T.final_act)[o] = make_double2(ax, ay);      // one 16-byte piece per lane, consecutive lanes on consecutive addresses
        }
        if (j == 0) { T.episode[env] = episode; T.choice[env] = kind; T.counter[env] = counter + 1; }
    }
    if (agent) {
        if (TEAM == SCRIPTED_CAMERAS) {
            if (a.record.camera_u) reinterpret_cast<double2 *>(a.record.camera_u)[o] = make_double2(rec[0], rec[1]);
        } else {
            if (a.record.target_u) { a.record.target_u[o * 3] = rec[0]; a.record.target_u[o * 3 + 1] = rec[1]; a.record.target_u[o * 3 + 2] = rec[2]; }
            if (a.record.target_reset) {
                reinterpret_cast<double2 *>(a.record.target_reset)[o * 2] = make_double2(rec_reset[0], rec_reset[1]);
                reinterpret_cast<double2 *>(a.record.target_reset)[o * 2 + 1] = make_double2(rec_reset[2], rec_reset[3]);
            }
        }
    }
    if (j == 0 && a.record.choice) a.record.choice[(int64_t)TEAM * N + env] = kind;
}

__global__ __launch_bounds__(256) void scripted_opponent_kernel(const Params *__restrict__ pp, const Ptrs g, const ScriptedArgs a) {
    extern __shared__ __align__(16) unsigned char scripted_lds[];
    const Params &p = *pp;
    const int Nc = p.Nc, Nt = p.Nt, DW = p.DW;
    const int tid = threadIdx.x, el = tid >> 4, j = tid & 15;
    const int64_t e0 = (int64_t)blockIdx.x * kAttachedEnvsPerBlock;
    if (e0 >= g.N) return;
    const int ne = (int)(g.N - e0 < (int64_t)kAttachedEnvsPerBlock ? g.N - e0 : (int64_t)kAttachedEnvsPerBlock);
    double *dy = reinterpret_cast<double *>(scripted_lds);
    stage_records(dy, g.dyn + e0 * DW, ne * DW, tid);
    const int64_t env = e0 + el;
    const bool live = el < ne;
    uint64_t capword = 0ull;
    if (live && a.team[SCRIPTED_TARGETS].on && j < Nt) capword = reinterpret_cast<const uint64_t *>(g.stat + env * p.SW)[3 * Nc + 3 * p.No];
    __syncthreads();
    if (!live) return;                                           // lanes beyond the batch: nothing below is theirs

    const double *d = dy + el * DW;
    const int32_t *di = reinterpret_cast<const int32_t *>(d + p.DF);
    const bool frozen = a.freeze_done && (di + Nt * TI_STRIDE)[EI_DONE] != 0;      // finished, waiting for the batched reset: the agents did not act
    scripted_team<SCRIPTED_CAMERAS>(p, a, g.N, d, di, env, j, frozen, capword);
    scripted_team<SCRIPTED_TARGETS>(p, a, g.N, d, di, env, j, frozen, capword);
}

hipError_t launch_scripted_opponents(unsigned blocks, size_t lds, hipStream_t stream, const Params *params, const Ptrs &g, const ScriptedArgs &a) {
    hipLaunchKernelGGL(scripted_opponent_kernel, dim3(blocks), dim3(256), lds, stream, params, g, a);
    return hipGetLastError();
}

}  // namespace mate
