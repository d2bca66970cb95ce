// selection_rows.hpp -- target-selection camera actions: the per-frame part of the reference's HierarchicalCamera wrapper
// (examples/hrl/wrappers.py) as launches attached to the engine.  The learner emits a SELECTION of targets per camera; a fixed
// executor (HierarchicalCamera.track, wrappers.py:183-220) turns it into the camera team's continuous joint action on every frame,
// from the cameras' true state, the selected targets' true positions and the cameras' view of the previous frame.  Not on the step
// path: launches of their own (mate_engine_enable_selection / mate_engine_step_selected), no stepping kernel is touched.
//
// One kernel, three phases chosen by launch argument:
//   SELECTION_EXECUTE      ahead of the stepping launch: actions [N][Nc][2] ActT into the engine-owned buffer the step reads
//   SELECTION_OBSERVE      behind the stepping (and reward) launch, ahead of the restart: the four metrics of wrappers.py:120-136
//                          against the masks of the step that has just run, [N][Nc][4] f64, and the frames that contributed [N]
//   SELECTION_ACTION_MASK  behind the restart: action_mask() (wrappers.py:166-175) of the observation the learner sees next
//
// view[c] is the opponent-flag column of camera c's observation row as the packer writes it: the camera_target_view_mask bits in
// plain mode, their OR over the cameras under SharedFieldOfView, all ones under EnhancedObservation.
//
// Mapping: the tile of attached_tile.hpp, lane j of a group is camera j; the camera locations of the static records are staged next
// to the dynamic records.  f64 throughout, product then add (-ffp-contract=off); fused where the Greedy agents' code fuses (norm2).
#pragma once
#include "attached_tile.hpp"
#include "policy_kernels.hpp"

namespace mate {

constexpr int kSelectionMetrics = 4;      // num_selected_targets | num_valid_selected_targets | num_invalid_selected_targets | invalid_target_selection_rate
enum SelectionPhase : int32_t { SELECTION_EXECUTE = 0, SELECTION_OBSERVE = 1, SELECTION_ACTION_MASK = 2 };

struct SelectionArgs {
    const void *selection;        // [N][Nc]: int32 index in [0, Nt] (Nt: none) or, `multi`, uint32 with bit t = target t selected
    void *actions;                // [N][Nc][2] ActT, engine-owned: the camera team's joint action of the stepping launch
    const uint32_t *masks;        // [N][MW]: the engine's own mask words, as the last step / reset / restart left them
    const float *scalars;         // observe: [N][8] of the step that has just run
    double *metrics;              // [N][Nc][4], or null
    int32_t *frames;              // [N], or null
    uint8_t *action_mask;         // [N][Nc][2 Nt] (multi: even entries 1) / [N][Nc][Nt + 1] (single: last entry 1), or null
    int32_t multi, cam_mode, accumulate;
    int32_t bit_ct;               // mate_layout.bit_camera_target
    int32_t phase;
};

// The viewing angle that puts `distance` at the rim of the sector (wrappers.py:207-210): best <- area_product / (distance (1 +
// sin(min(best / 2, 90))))^2, 20 times from 180 -- the reference's operations in the reference's order (zoom_fixed_point of the Greedy
// agents takes the quotient as K (1 / (1 + sin))^2: the same fixed point, other roundings).
__device__ __forceinline__ double selection_zoom(double area_product, double distance) {
    double best = 180.0;
    for (int it = 0; it < kZoomIterations; ++it) {
        const double half = best / 2.0;
        const double sight = distance * (1.0 + sin_deg_0_90(half < 90.0 ? half : 90.0));
        best = div_nz(area_product, sight * sight);
    }
    return best;
}

template <typename ActT>
__global__ __launch_bounds__(256) void selection_kernel(const Params *__restrict__ pp, const Ptrs g, const SelectionArgs a) {
    extern __shared__ __align__(16) unsigned char selection_lds[];
    __shared__ uint32_t mask_words[kAttachedEnvsPerBlock][16];
    __shared__ double cam_xy[kAttachedEnvsPerBlock][32];
    const Params &p = *pp;
    const int Nc = p.Nc, Nt = p.Nt, DW = p.DW;
    const int tid = threadIdx.x, el = tid >> 4, j = tid & 15;
    const int64_t e0 = (int64_t)blockIdx.x * kAttachedEnvsPerBlock;
    if (e0 >= g.N) return;
    const int ne = (int)(g.N - e0 < (int64_t)kAttachedEnvsPerBlock ? g.N - e0 : (int64_t)kAttachedEnvsPerBlock);
    double *dy = reinterpret_cast<double *>(selection_lds);
    if (a.phase == SELECTION_EXECUTE) {      // the camera locations: 2 Nc words per static record
        stage_records(dy, g.dyn + e0 * DW, ne * DW, tid);
        for (int i = tid; i < ne * 32; i += 256) { const int e = i >> 5, k = i & 31; if (k < 2 * Nc) cam_xy[e][k] = g.stat[(e0 + e) * p.SW + k]; }
    }
    const int64_t env = e0 + el;
    const bool live = el < ne, is_cam = j < Nc;
    const ViewWords vw = view_words(a.bit_ct, Nc, Nt);
    float scalar = 0.f;
    if (live) {
        if (a.phase == SELECTION_OBSERVE) scalar = a.scalars[env * 8 + (j & 7)];
        load_view_words(mask_words[el], vw, a.masks, env, p.MW, j);
    }
    __syncthreads();
    if (!live) return;

    const uint32_t all = (1u << Nt) - 1u;      // (Nt <= 16)
    uint32_t view = is_cam ? view_row(mask_words[el], vw, j, Nt) : 0u;
    if (a.cam_mode == 2) {                     // SharedFieldOfView: what any camera sees
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) view |= (uint32_t)__shfl_xor((int)view, off, 16);
    } else if (a.cam_mode == 1) view = all;    // EnhancedObservation: every flag is set
    const bool idle = a.phase == SELECTION_OBSERVE && tile_idle(scalar);
    if (!is_cam) return;

    if (a.phase == SELECTION_ACTION_MASK) {
        if (!a.action_mask) return;
        if (a.multi) {
            uint8_t *out = a.action_mask + (env * Nc + j) * (2 * Nt);
            for (int t = 0; t < Nt; ++t) { out[2 * t] = 1; out[2 * t + 1] = (uint8_t)((view >> t) & 1u); }
        } else {
            uint8_t *out = a.action_mask + (env * Nc + j) * (Nt + 1);
            for (int t = 0; t < Nt; ++t) out[t] = (uint8_t)((view >> t) & 1u);
            out[Nt] = 1;
        }
        return;
    }

    uint32_t sel;
    if (a.multi) sel = reinterpret_cast<const uint32_t *>(a.selection)[env * Nc + j] & all;
    else { const int idx = reinterpret_cast<const int32_t *>(a.selection)[env * Nc + j]; sel = (idx >= 0 && idx < Nt) ? 1u << idx : 0u; }   // index2onehot: row Nt is all zero
    const uint32_t valid = sel & view;

    if (a.phase == SELECTION_OBSERVE) {        // wrappers.py:120-136
        if (idle && a.accumulate) return;      // contributes nothing, its count does not move
        const int n_sel = __popc(sel), n_valid = __popc(valid), n_invalid = __popc(sel & ~view);
        double m[kSelectionMetrics] = {(double)n_sel, (double)n_valid, (double)n_invalid, (double)n_invalid / (double)(n_sel > 1 ? n_sel : 1)};
        if (a.metrics) {
            double *out = a.metrics + (env * Nc + j) * kSelectionMetrics;
#pragma unroll
            for (int k = 0; k < kSelectionMetrics; ++k) out[k] = idle ? 0.0 : a.accumulate ? out[k] + m[k] : m[k];
        }
        if (a.frames && j == 0) a.frames[env] = idle ? 0 : a.accumulate ? a.frames[env] + 1 : 1;
        return;
    }

    // HierarchicalCamera.track (wrappers.py:183-220)
    double a0 = -p.rot, a1 = -p.zoom;          // no valid target: camera.action_space.low
    if (valid) {
        const double *d = dy + el * DW;
        double sx = 0.0, sy = 0.0;
        for (uint32_t m = valid; m != 0u; m &= m - 1u) {      // np.mean(axis=0): the rows added in target order, then one division
            const int t = __ffs((int)m) - 1;
            sx = sx + d[2 * Nc + t]; sy = sy + d[2 * Nc + Nt + t];
        }
        const double n = (double)__popc(valid);
        const double dx = div_nz(sx, n) - cam_xy[el][j], dyc = div_nz(sy, n) - cam_xy[el][Nc + j];
        const double phi = d[j], theta = d[Nc + j];
        const double orientation = (dx == 0.0 && dyc == 0.0) ? 0.0 : atan2_deg(dyc, dx);
        const double distance = norm2(dx, dyc);
        double best;
        if (distance * (1.0 + sin_deg_0_90(p.theta_min / 2.0)) >= p.rmax) best = p.theta_min;
        else {
            const double sight = sqrt_pos(div_nz(p.area, theta));      // Camera.sight_range (entities.py:360)
            const double area_product = theta * (sight * sight);
            if (distance <= sqrt_pos(area_product / 180.0) / 2.0) best = 180.0;
            else best = clipd(selection_zoom(area_product, distance), p.theta_min, 180.0);
        }
        a0 = clipd(normalize_angle(orientation - phi), -p.rot, p.rot);
        a1 = clipd(best - theta, -p.zoom, p.zoom);
    }
    ActT *out = reinterpret_cast<ActT *>(a.actions) + (env * Nc + j) * 2;
    out[0] = (ActT)a0; out[1] = (ActT)a1;
}

}  // namespace mate
