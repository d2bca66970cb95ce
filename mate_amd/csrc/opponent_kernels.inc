// opponent_kernels.inc -- heuristic_drift_kernel and its launch function (opponent_rows.hpp describes both).  Included exactly once per library: by
// opponent_kernels.hip (mate_amd/build.py), or by mate_engine.hip in the single-unit build.
#include "opponent_rows.hpp"

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

}  // namespace mate
