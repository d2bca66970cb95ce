// state_rows.hpp -- the global state row of every environment, MultiAgentTracking.state() (environment.py:894-906 of the
// reference): what a centralised critic (MAPPO, MADDPG, QMIX-style mixers, I2C, TarMAC: examples/utils/wrappers.py:170-225)
// is trained on.  One row of S = 13 + 9 Nc + 14 Nt + 3 No + 2 Nt + 16 reals per environment, in the reference's order:
//
//   preserved_data (13) | per camera state(private=True) (9) | per target state(private=True) (14) | per obstacle state() (3)
//   | freights (Nt) | bounties (Nt) | remaining_cargoes (16)
//
// preserved_data[3] (the agent index of an observation row) stays 0.  Not on the step path: a launch of its own behind the
// launches that leave new records (mate_engine_enable_state_rows), or on demand (mate_engine_state_rows).
//
// A workgroup owns a TILE of E consecutive environments (E a multiple of 4).  Their static and dynamic records are two
// contiguous stretches of HBM, staged in LDS with whole-wave 8-byte-per-lane loads; the rows are assembled in LDS, as the flat
// [E][S] image of the tile's stretch of the output, by one lane per ENTITY (a camera lane writes its nine values, a target lane
// its fourteen ...: straight-line code per class, no per-element decode); an optional pass applies the per-element (scale, bias);
// the image leaves as consecutive 16-byte chunks.  S * sizeof(OutT) is in general no multiple of 16 (S = 81, 111, 193, 253 ...),
// E * S * sizeof(OutT) always is: every tile begins on a 16-byte boundary of the densely packed output and only the last,
// partial tile of the whole array can end with fewer than 16 bytes, which leave as scalar stores.
//
// The derived entries are computed as the observation packer computes an agent's own private state (simulate_cameras,
// fill_scratch in engine_kernels.hpp: the same device_math.hpp functions on the same record words, the same casts), so that a
// raw row's camera / target blocks are bit-identical to elements [13:22] / [13:27] of that agent's plain observation row of the same type.
#pragma once
#include "attached_tile.hpp"

namespace mate {

constexpr int kStateTailFixed = 16;      // remaining_cargoes: NUM_WAREHOUSES^2
__host__ __device__ constexpr int state_dim_of(int Nc, int Nt, int No) { return 13 + 9 * Nc + 14 * Nt + 3 * No + 2 * Nt + kStateTailFixed; }   // environment.py:450-466
__host__ __device__ constexpr int state_rows_record_bytes(int SW, int DW, int E) { return shape_round_up(E * (SW + DW) * 8, 16); }
__host__ __device__ constexpr int state_rows_lds_bytes(int SW, int DW, int S, int E, int out_size) {
    return state_rows_record_bytes(SW, DW, E) + shape_round_up(E * S * out_size, 16);
}

// Camera.state's polar2cartesian(sight_range, orientation) (entities.py:318, 360) -- simulate_cameras' own sequence for each row type
template <typename OutT>
__device__ __forceinline__ void camera_sight_xy(double area, double ph, double th, OutT &x, OutT &y) {
    const double sr2 = div_nz(area, th);
    if constexpr (sizeof(OutT) == 4) {
        float sn, cs;
        sincos_deg_f32(ph, sn, cs);
        const float srf = sqrt_f32_1ulp((float)sr2);
        x = srf * cs; y = srf * sn;
    } else {
        const double sr = sqrt_pos(sr2);
        double sn, cs;
        sincos_deg(ph, sn, cs);
        x = (OutT)(sr * cs); y = (OutT)(sr * sn);
    }
}

// `ab`: interleaved (scale, bias) per row element, or null for the raw row.  `E`: environments per workgroup.
template <typename OutT>
__global__ __launch_bounds__(256) void state_rows_kernel(const Params *__restrict__ pp, const Ptrs g, OutT *__restrict__ dst,
                                                         const OutT *__restrict__ ab, const int32_t E) {
    extern __shared__ __align__(16) unsigned char state_lds[];
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const Params &p = *pp;
    const int Nc = p.Nc, Nt = p.Nt, No = p.No, SW = p.SW, DW = p.DW;
    const int S = state_dim_of(Nc, Nt, No);
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * E;
    if (e0 >= g.N) return;
    const int ne = (int)(g.N - e0 < (int64_t)E ? g.N - e0 : (int64_t)E);
    double *st = reinterpret_cast<double *>(state_lds);
    double *dy = st + E * SW;
    OutT *tile = reinterpret_cast<OutT *>(state_lds + state_rows_record_bytes(SW, DW, E));

    stage_records(st, g.stat + e0 * SW, ne * SW, tid);      // the tile's records: two contiguous stretches
    stage_records(dy, g.dyn + e0 * DW, ne * DW, tid);
    __syncthreads();

    for (int item = tid; item < ne * Nc; item += 256) {           // Camera.state(private=True), entities.py:313-321
        const int el = item / Nc, c = item - el * Nc;
        const double *s = st + el * SW, *d = dy + el * DW;
        OutT *row = tile + el * S + 13 + 9 * c;
        OutT x, y;
        camera_sight_xy<OutT>(p.area, d[c], d[Nc + c], x, y);
        row[0] = (OutT)s[c]; row[1] = (OutT)s[Nc + c]; row[2] = (OutT)p.cam_radius;
        row[3] = x; row[4] = y; row[5] = (OutT)d[Nc + c];
        row[6] = (OutT)p.rmax; row[7] = (OutT)p.rot; row[8] = (OutT)p.zoom;
    }
    for (int item = tid; item < ne * Nt; item += 256) {           // Target.state(private=True), entities.py:631-637 (fill_scratch)
        const int el = item / Nt, t = item - el * Nt;
        const double *s = st + el * SW, *d = dy + el * DW;
        const int32_t *di = reinterpret_cast<const int32_t *>(d + p.DF);
        OutT *row = tile + el * S + 13 + 9 * Nc + 14 * t;
        const int gw = di[t * TI_STRIDE + TI_GW] & 0xffffff;      // bit 24 (colliding) is not part of the state
        const int cap = 1 + (int)((reinterpret_cast<const uint64_t *>(s)[3 * Nc + 3 * No] >> t) & 1ull);
        const int goal = (gw & 0xff) - 1, weight = (gw >> 8) & 0xff, empty = (gw >> 16) & 0xf;
        row[0] = (OutT)d[2 * Nc + t]; row[1] = (OutT)d[2 * Nc + Nt + t]; row[2] = (OutT)p.tgt_sight;
        row[3] = (OutT)(goal >= 0 && weight > 0 ? 1.0 : 0.0);
        row[4] = (OutT)(cap == 2 ? p.tgt_step * 0.5 : p.tgt_step); row[5] = (OutT)cap;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            row[6 + w] = (OutT)(goal == w ? weight : 0);
            row[10 + w] = (OutT)((empty >> w) & 1);
        }
    }
    for (int item = tid; item < ne * No; item += 256) {           // Obstacle.state, entities.py:147-148
        const int el = item / No, o = item - el * No;
        const double *s = st + el * SW + 2 * Nc;
        OutT *row = tile + el * S + 13 + 9 * Nc + 14 * Nt + 3 * o;
        row[0] = (OutT)s[o]; row[1] = (OutT)s[No + o]; row[2] = (OutT)s[2 * No + o];
    }
    {   // preserved_data (environment.py:499-501) in front, freights | bounties | remaining_cargoes behind: one value per lane
        const int tail = 2 * Nt + kStateTailFixed, H = 13 + tail;
        for (int item = tid; item < ne * H; item += 256) {
            const int el = item / H, k = item - el * H;
            const int32_t *di = reinterpret_cast<const int32_t *>(dy + el * DW + p.DF);
            OutT *row = tile + el * S;
            if (k < 13) {
                // Nc, Nt, No, 0, the four warehouse centres (+-925: constants.py:70-72; x y of warehouses 0..3, minus signs at 2 4 5 7), radius 75
                const double v = k == 0 ? (double)Nc : k == 1 ? (double)Nt : k == 2 ? (double)No : k == 3 ? 0.0
                                 : k == 12 ? 75.0 : (((0xB4 >> (k - 4)) & 1) ? -925.0 : 925.0);
                row[k] = (OutT)v;
            } else {
                const int q = k - 13;
                const int word = q < Nt ? q * TI_STRIDE + TI_FREIGHT : q < 2 * Nt ? (q - Nt) * TI_STRIDE + TI_BOUNTY : Nt * TI_STRIDE + EI_REMAINING + (q - 2 * Nt);
                row[S - tail + q] = (OutT)di[word];
            }
        }
    }
    __syncthreads();

    if (ab) {      // normalize_observation (agents/utils.py:97-127) as one affine map per element: x * scale + bias, no fma (-ffp-contract=off)
        const int lane = tid & 63;
        for (int el = tid >> 6; el < ne; el += 4)
            for (int j = lane; j < S; j += 64) tile[el * S + j] = tile[el * S + j] * ab[2 * j] + ab[2 * j + 1];
        __syncthreads();
    }

    // the tile's stretch of the flat output: 16-byte chunks, a kilobyte per wave and store
    const int64_t first = e0 * S;                                  // (element index: a multiple of 16 bytes, see above)
    const int elems = ne * S, chunks = (int)((size_t)elems * sizeof(OutT) / 16);
    f32x4 *out = reinterpret_cast<f32x4 *>(dst + first);
    const f32x4 *in = reinterpret_cast<const f32x4 *>(tile);
    for (int q = tid; q < chunks; q += 256) stream_store(in[q], out + q);
    const int done = chunks * (int)(16 / sizeof(OutT));            // the last < 16 bytes of the WHOLE array (a partial last tile only)
    if (tid < elems - done) dst[first + done + tid] = tile[done + tid];
}

}  // namespace mate
