// opponent_kernels.hip -- heuristic_drift_kernel, heuristic_camera_kernel and their launch functions (opponent_rows.hpp describes them): the opponents' kernels
// beyond the Greedy pair, both teams', as a translation unit of its own; and fragment_frame_kernel (frame_rows.hpp), the per-frame FrameSkip fragment that
// makes those opponents usable under frame_skip > 1.  Their kernel-resource remarks are kept apart from the other units'
// (mate_amd/build.py: lib/kernel_resources_opponents.json).
#include <hip/hip_runtime.h>
#include "opponent_rows.hpp"
#include "frame_rows.hpp"

namespace mate {

__global__ __launch_bounds__(256) void heuristic_drift_kernel(const Params *__restrict__ pp, const Ptrs g, const DriftArgs a) {
    extern __shared__ __align__(16) unsigned char drift_lds[];
    __shared__ double cam_xy[kAttachedEnvsPerBlock][32];
    const Params &p = *pp;
    const int Nc = p.Nc, Nt = p.Nt, DW = p.DW;
    const int tid = threadIdx.x, el = tid >> 4, j = tid & 15;
    const int64_t e0 = (int64_t)blockIdx.x * kAttachedEnvsPerBlock;
    if (e0 >= g.N) return;
    const int ne = (int)(g.N - e0 < (int64_t)kAttachedEnvsPerBlock ? g.N - e0 : (int64_t)kAttachedEnvsPerBlock);
    double *dy = reinterpret_cast<double *>(drift_lds);
    stage_records(dy, g.dyn + e0 * DW, ne * DW, tid);
    for (int i = tid; i < ne * 32; i += 256) { const int e = i >> 5, k = i & 31; if (k < 2 * Nc) cam_xy[e][k] = g.stat[(e0 + e) * p.SW + k]; }
    const int64_t env = e0 + el;
    const bool live = el < ne, is_tgt = j < Nt;
    uint32_t sensed = 0u;
    uint64_t capword = 0ull;
    double gx = 0.0, gy = 0.0;
    if (live && is_tgt) {
        if (Nc > 0) {             // row j of the target rows: Nc <= 16 bits from bit_tr + j NJ, in at most two words
            const int b = a.bit_tr + j * p.NJ, w = b >> 5;
            const uint32_t *m = a.masks + env * p.MW;
            const uint64_t lo = m[w], hi = w + 1 < p.MW ? m[w + 1] : 0u;
            sensed = (uint32_t)((lo | (hi << 32)) >> (b & 31)) & ((1u << Nc) - 1u);
        }
        capword = reinterpret_cast<const uint64_t *>(g.stat + env * p.SW)[3 * Nc + 3 * p.No];
        gx = a.greedy[(env * Nt + j) * 2]; gy = a.greedy[(env * Nt + j) * 2 + 1];
    }
    __syncthreads();
    if (!live || !is_tgt) return;

    const double *d = dy + el * DW;
    const int32_t *di = reinterpret_cast<const int32_t *>(d + p.DF);
    const bool frozen = a.freeze_done && (di + Nt * TI_STRIDE)[EI_DONE] != 0;      // finished, waiting for the batched reset: the agents did not act
    double outx = gx, outy = gy;
    if (!frozen && sensed) {
        const double step_size = ((capword >> j) & 1ull) ? p.tgt_step * 0.5 : p.tgt_step;
        const double tx = d[2 * Nc + j], ty = d[2 * Nc + Nt + j];
        bool found = false;
        double best = 0.0, bx = 0.0, by = 0.0;
        for (uint32_t m = sensed; m != 0u; m &= m - 1u) {
            const int c = __ffs((int)m) - 1;
            const double cx = cam_xy[el][c], cy = cam_xy[el][Nc + c];
            const double phi = normalize_angle(d[c]), theta = d[Nc + c];      // (the observation's orientation is an atan2: in (-180, 180])
            const double dx = tx - cx, dyc = ty - cy;
            const double half = theta / 2.0;
            const double sight = sqrt_pos(div_nz(p.area, theta));             // Camera.sight_range (entities.py:360)
            const double angle = (dx == 0.0 && dyc == 0.0) ? 0.0 : atan2_deg(dyc, dx);
            const double angle_diff = normalize_angle(angle - phi);
            if (norm2(dx, dyc) <= 1.2 * sight && angle_diff <= 1.2 * half) {
                const double reach = div_nz(sight, 1.0 + sin_deg_0_90(half < 90.0 ? half : 90.0));
                double sn, cs;
                sincos_deg(phi, sn, cs);
                const double ex = cx + reach * cs, ey = cy + reach * sn;
                const double inner = sight - reach;
                const double rel = div_nz(norm2(tx - ex, ty - ey), inner);
                if (!found || rel < best) { found = true; best = rel; bx = ex; by = ey; }      // min(): the first minimum
            }
        }
        if (found) {
            double fx = tx - bx, fy = ty - by;
            const double size = norm2(fx, fy), cap = step_size * a.noise_scale;
            if (size > cap) { const double k = div_nz(cap, size); fx *= k; fy *= k; }
            if (gx * fx + gy * fy >= 0.0) { outx = clipd(gx + fx, -step_size, step_size); outy = clipd(gy + fy, -step_size, step_size); }
        }
    }
    a.final_act[(env * Nt + j) * 2] = outx; a.final_act[(env * Nt + j) * 2 + 1] = outy;
}

hipError_t launch_heuristic_drift(unsigned blocks, size_t lds, hipStream_t stream, const Params *params, const Ptrs &g, const DriftArgs &a) {
    hipLaunchKernelGGL(heuristic_drift_kernel, dim3(blocks), dim3(256), lds, stream, params, g, a);
    return hipGetLastError();
}

// (value, index) argmin over a wave: every lane ends with the winner, the lowest index among equal values
__device__ __forceinline__ void hc_wave_argmin(double &v, int &i) {
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}
__global__ __launch_bounds__(256) void heuristic_camera_kernel(const Params *__restrict__ pp, const Ptrs g, const HeuristicCameraArgs a) {
    extern __shared__ __align__(16) unsigned char hc_lds[];
    __shared__ int8_t perm[kHcPermutations][kHcMaxAgents];
    __shared__ uint8_t pair_t[kHcMaxAgents][kHcMaxAgents];       // camera c's in-range targets in list order
    __shared__ int16_t pair_g[kHcMaxAgents][kHcMaxAgents];       // ... and their nearest grid points
    __shared__ int32_t cnt[kHcMaxAgents];
    __shared__ uint32_t seen[kHcMaxAgents];
    __shared__ double cam_px[kHcMaxAgents], cam_py[kHcMaxAgents], cam_phi[kHcMaxAgents], cam_theta[kHcMaxAgents], tgx[kHcMaxAgents], tgy[kHcMaxAgents];
    __shared__ double res_total[kHcPermutations], res_cost[kHcPermutations];
    __shared__ int16_t res_idx[kHcPermutations][kHcMaxAgents];
    __shared__ int32_t winner;
    __shared__ double mesh_o[36], mesh_a[21];                    // state s = a 36 + o: the mesh's orientation and viewing-angle columns
    const Params &p = *pp;
    const int Nc = p.Nc, Nt = p.Nt;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t env = blockIdx.x;
    if (env >= g.N) return;
    const double *d = g.dyn + env * p.DW;
    const int32_t *env_i = reinterpret_cast<const int32_t *>(d + p.DF) + Nt * TI_STRIDE;
    if (a.freeze_done && env_i[EI_DONE] != 0) return;      // finished, waiting for the batched reset: the agents do not act
    const uint32_t tick = (uint32_t)env_i[EI_TICK];
    const uint32_t env_global = p.first_env + (uint32_t)env;
    const int32_t episode = env_i[EI_EPISODE];

    // ---------------------------------------------------------------------------------------------- 0: records, permutations, the grid
    double prev0 = 0.0, prev1 = 0.0;
    if (tid < Nc) {
        const int c = tid;
        const double *st = g.stat + env * p.SW;
        cam_px[c] = st[c]; cam_py[c] = st[Nc + c]; cam_phi[c] = d[c]; cam_theta[c] = d[Nc + c];
        const int b = c * Nt, w = b >> 5;      // row c of camera_target_view_mask: bits [c Nt, c Nt + Nt) of the packed words
        const uint32_t *m = a.masks + env * p.MW;
        const uint64_t lo = m[w], hi = w + 1 < p.MW ? m[w + 1] : 0u;
        seen[c] = (uint32_t)((lo | (hi << 32)) >> (b & 31)) & ((1u << Nt) - 1u);
        if (a.episode[env] == episode) { prev0 = a.prev_action[(env * Nc + c) * 2]; prev1 = a.prev_action[(env * Nc + c) * 2 + 1]; }      // else: the agents' reset
    } else if (tid >= 32 && tid < 32 + Nt) {
        const int t = tid - 32;
        tgx[t] = d[2 * Nc + t]; tgy[t] = d[2 * Nc + Nt + t];
    } else if (tid >= 64 && tid < 64 + kHcPermutations) {
        const int k = tid - 64;
        const int64_t row = (env * kHcPermutations + k) * Nc;
        if (a.permutations) {
            for (int j = 0; j < Nc; ++j) { int v = a.permutations[row + j]; v = v < 0 ? 0 : (v >= Nc ? Nc - 1 : v); perm[k][j] = (int8_t)v; }
        } else {
            const U4 r0 = philox(p.seed_lo, p.seed_hi, env_global, tick, S_HCAM_PERM, (uint32_t)(2 * k));
            const U4 r1 = philox(p.seed_lo, p.seed_hi, env_global, tick, S_HCAM_PERM, (uint32_t)(2 * k + 1));
            const uint64_t w0 = (uint64_t)r0.x | ((uint64_t)r0.y << 32), w1 = (uint64_t)r0.z | ((uint64_t)r0.w << 32);
            const uint64_t w2 = (uint64_t)r1.x | ((uint64_t)r1.y << 32), w3 = (uint64_t)r1.z | ((uint64_t)r1.w << 32);
            for (int j = 0; j < Nc; ++j) perm[k][j] = (int8_t)j;
            for (int i = Nc - 1; i >= 1; --i) {
                const int n = Nc - 1 - i, q4 = n >> 2;
                const uint64_t word = q4 == 0 ? w0 : (q4 == 1 ? w1 : (q4 == 2 ? w2 : w3));
                const uint32_t u = (uint32_t)(word >> (16 * (n & 3))) & 0xffffu;
                const int j = (int)((u * (uint32_t)(i + 1)) >> 16);
                const int8_t x = perm[k][i]; perm[k][i] = perm[k][j]; perm[k][j] = x;
            }
        }
        if (a.record) for (int j = 0; j < Nc; ++j) a.record[row + j] = perm[k][j];
    }
    if (tid >= 128 && tid < 128 + 36) mesh_o[tid - 128] = a.mesh[3 * (tid - 128)];
    else if (tid >= 192 && tid < 192 + 21) mesh_a[tid - 192] = a.mesh[3 * 36 * (tid - 192) + 1];
    double *grid = reinterpret_cast<double *>(hc_lds);
    {   // the grid, twelve 16-byte loads per thread in flight at once
        const double2 *src = reinterpret_cast<const double2 *>(a.grid);
        double2 *dst = reinterpret_cast<double2 *>(hc_lds);
        double2 held[11];      // (2952 = 11 * 256 + 136)
#pragma unroll
        for (int m = 0; m < 11; ++m) held[m] = src[tid + 256 * m];
        const int tail = tid + 256 * 11;
        double2 last = held[0];
        if (tail < kHcPoints) last = src[tail];
#pragma unroll
        for (int m = 0; m < 11; ++m) dst[tid + 256 * m] = held[m];
        if (tail < kHcPoints) dst[tail] = last;
    }
    __syncthreads();

    // the sensed targets in insertion order; camera `tid` keeps those within its range
    if (tid < Nc) {
        const int c = tid;
        const double cx = cam_px[c], cy = cam_py[c];
        uint32_t listed = 0u;
        int n = 0;
        for (int o = 0; o < Nc; ++o) {
            for (uint32_t m = seen[o] & ~listed; m != 0u; m &= m - 1u) {
                const int t = __ffs((int)m) - 1;
                if (norm2(tgx[t] - cx, tgy[t] - cy) <= p.rmax) pair_t[c][n++] = (uint8_t)t;
            }
            listed |= seen[o];
        }
        cnt[c] = n;
    }
    __syncthreads();

    // ---------------------------------------------------------------------------------------------- 1: the nearest grid point of every pair
    for (int slot = wave; slot < Nc * kHcMaxAgents; slot += 4) {
        const int c = slot >> 4, k = slot & 15;
        if (k >= __builtin_amdgcn_readfirstlane(cnt[c])) continue;
        const int t = pair_t[c][k];
        const double dx = tgx[t] - cam_px[c], dy = tgy[t] - cam_py[c];
        double best = 1.0e300;
        int bi = lane;
#pragma unroll 4
        for (int q = lane; q < kHcPoints; q += 64) {
            const double ex = dx - grid[2 * q], ey = dy - grid[2 * q + 1];
            const double d2 = ex * ex + ey * ey;
            // a smaller square wins where its root is smaller too: certainly beyond 2^-50 relative, else the correctly rounded roots say
            if (d2 < best && (d2 < best * (1.0 - 0x1p-50) || __builtin_sqrt(d2) < __builtin_sqrt(best))) { best = d2; bi = q; }
        }
        double root = __builtin_sqrt(best);
        hc_wave_argmin(root, bi);
        if (lane == 0) pair_g[c][k] = (int16_t)bi;
    }
    __syncthreads();      // (the grid has been read: its bytes become the accumulators)

    // ---------------------------------------------------------------------------------------------- 2: scores_c and bits_c
    double *sc = reinterpret_cast<double *>(hc_lds);
    uint16_t *bt = reinterpret_cast<uint16_t *>(hc_lds + (size_t)Nc * kHcStates * 8);
    {   // thread tid holds states tid, tid + 256 and (tid < 244) tid + 512: three independent loads per row in flight
        const int s0 = tid, s1 = tid + 256, s2 = tid + 512;
        const bool third = s2 < kHcStates;
        for (int c = 0; c < Nc; ++c) {
            double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
            uint32_t bits0 = 0u, bits1 = 0u, bits2 = 0u;
            const int n = cnt[c];
#pragma unroll 4
            for (int k = 0; k < n; ++k) {
                const double *row = a.scores + (int64_t)pair_g[c][k] * kHcStates;
                const uint32_t bit = 1u << pair_t[c][k];
                const double v0 = row[s0], v1 = row[s1], v2 = third ? row[s2] : 0.0;
                acc0 += v0; acc1 += v1; acc2 += v2;
                if (v0 > 0.0) bits0 |= bit;
                if (v1 > 0.0) bits1 |= bit;
                if (v2 > 0.0) bits2 |= bit;
            }
            sc[c * kHcStates + s0] = acc0; bt[c * kHcStates + s0] = (uint16_t)bits0;
            sc[c * kHcStates + s1] = acc1; bt[c * kHcStates + s1] = (uint16_t)bits1;
            if (third) { sc[c * kHcStates + s2] = acc2; bt[c * kHcStates + s2] = (uint16_t)bits2; }
        }
    }
    __syncthreads();

    // ---------------------------------------------------------------------------------------------- 3: eight greedy assignments per wave, at once
    {   // eight lanes per permutation: the wave's eight chains of picks run side by side, a pick's reduction is three steps within the group
        const int sub = lane & 7, k = wave * 8 + (lane >> 3);
        uint32_t cur = 0u;
        double total = 0.0, cost = 0.0;
        for (int j = 0; j < Nc; ++j) {
            const int c = perm[k][j];
            const double *scc = sc + c * kHcStates;
            const uint16_t *btc = bt + c * kHcStates;
            double bv = -1.0;
            int i = 0;      // (a camera without in-range targets: scores and bits are zeros, the first maximum is state 0)
            if (cnt[c] > 0)
#pragma unroll 8
                for (int s = sub; s < kHcStates; s += 8) {
                    const double v = scc[s] + (double)__popc((uint32_t)btc[s] & ~cur);
                    if (v > bv) { bv = v; i = s; }
                }
            for (int off = 4; off > 0; off >>= 1) {      // the lowest index among equal values; every lane of the group ends with the winner
                const double ov = __shfl_xor(bv, off);
                const int oi = __shfl_xor(i, off);
                if (ov > bv || (ov == bv && oi < i)) { bv = ov; i = oi; }
            }
            const int ia = (int)(((unsigned)i * 1821u) >> 16);      // i / 36 for i < 756
            const double mo = mesh_o[i - 36 * ia], ma = mesh_a[ia];
            const double co = __builtin_fabs(mo - cam_phi[c]) / p.rot, ca = __builtin_fabs(ma - cam_theta[c]) / p.zoom;
            cost += co > ca ? co : ca;
            cur |= (uint32_t)btc[i];
            total += scc[i];
            if (sub == 0) res_idx[k][j] = (int16_t)i;
        }
        total += (double)__popc(cur);
        if (sub == 0) { res_total[k] = total; res_cost[k] = cost; }
    }
    __syncthreads();

    // ---------------------------------------------------------------------------------------------- 4: the winner, the goals, act()
    if (tid == 0) {
        int b = 0;
        for (int k = 1; k < kHcPermutations; ++k) {
            bool better = res_total[k] > res_total[b];
            if (!better && res_total[k] == res_total[b]) {
                better = res_cost[k] < res_cost[b];
                if (!better && res_cost[k] == res_cost[b])
                    for (int j = 0; j < Nc; ++j)
                        if (perm[k][j] != perm[b][j]) { better = perm[k][j] > perm[b][j]; break; }
            }
            if (better) b = k;
        }
        winner = b;
        a.episode[env] = episode;
    }
    if (tid < Nc) { cam_px[tid] = prev0; cam_py[tid] = prev1; }      // (the locations are done with: camera tid's previous action, for the thread that writes its row)
    __syncthreads();
    if (tid < Nc) {
        const int w = winner, c = perm[w][tid], i = res_idx[w][tid];      // position `tid` of the winning permutation
        const bool has = cnt[c] > 0;
        const int64_t o = env * Nc + c;
        double a0, a1, g0 = __builtin_nan(""), g1 = __builtin_nan("");
        if (has) {
            g0 = mesh_o[i % 36]; g1 = mesh_a[i / 36];
            a0 = clipd(normalize_angle(g0 - cam_phi[c]), -p.rot, p.rot);
            a1 = clipd(g1 - cam_theta[c], -p.zoom, p.zoom);
        } else {
            double u, u0, u1;
            if (a.binom_u && a.sample_u) { u = a.binom_u[o]; u0 = a.sample_u[o * 2]; u1 = a.sample_u[o * 2 + 1]; }
            else {
                const U4 r = philox(p.seed_lo, p.seed_hi, env_global, tick, S_HCAM_ACT, (uint32_t)c);
                u = (double)r.y * 2.3283064365386963e-10; u0 = (double)r.z * 2.3283064365386963e-10; u1 = (double)r.w * 2.3283064365386963e-10;
                if (a.binom_u) u = a.binom_u[o];
                if (a.sample_u) { u0 = a.sample_u[o * 2]; u1 = a.sample_u[o * 2 + 1]; }
            }
            if (u > 1.0 - 0.1) { a0 = -p.rot + (2.0 * p.rot) * u0; a1 = -p.zoom + (2.0 * p.zoom) * u1; }      // np_random.binomial(1, 0.1), action_space.sample()
            else { a0 = cam_px[c]; a1 = cam_py[c]; }
        }
        a.goals[o * 2] = g0; a.goals[o * 2 + 1] = g1;
        a.goal_index[o] = has ? i : -1;
        a.action[o * 2] = a0; a.action[o * 2 + 1] = a1;
        a.prev_action[o * 2] = a0; a.prev_action[o * 2 + 1] = a1;
    }
}

hipError_t launch_heuristic_camera(unsigned blocks, size_t lds, hipStream_t stream, const Params *params, const Ptrs &g, const HeuristicCameraArgs &a) {
    hipLaunchKernelGGL(heuristic_camera_kernel, dim3(blocks), dim3(256), lds, stream, params, g, a);
    return hipGetLastError();
}
const void *heuristic_camera_function() { return reinterpret_cast<const void *>(heuristic_camera_kernel); }

hipError_t launch_fragment_frame(bool obs_f64, unsigned blocks, hipStream_t stream, const FrameArgs &a) {
    if (obs_f64) hipLaunchKernelGGL(fragment_frame_kernel<double>, dim3(blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(fragment_frame_kernel<float>, dim3(blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace mate
