// info_rows.hpp -- what the reference's MoreTrainingInformation wrapper (wrappers/more_training_information.py:42-98 over environment.py:1271-1324)
// adds to every agent's info at a step, for every environment, as three f64 outputs; integers and booleans are stored exactly as doubles.
// Not on the step path: ONE launch of its own (mate_engine_enable_info_rows) behind the stepping launch and the reward launch and AHEAD of the
// restart, so that the rows describe the step the scalar record describes, the terminal one included.
//
//   camera row [N][Nc][2]    0 num_tracked = camera_target_view_mask[c, :].sum()     1 is_sensed = target_camera_view_mask[:, c].any()
//   target row [N][Nt][9]    0 goal (-1: none)    1 goal_distance = warehouse_distances[goal], or 1000 (TERRAIN_WIDTH / 2) without a goal
//                            2 .. 5 warehouse_distances = max(|location - WAREHOUSES[w]| - 75, 0): dx dx + dy dy, the root, the subtraction (-ffp-contract=off)
//                            6 individual_done = target_dones[t]: the goal differs from the goal before this step and that goal was >= 0
//                            7 is_tracked = camera_target_view_mask[:, t].any()      8 is_colliding
//   cargo row  [N][24]       0 .. 3 remaining_cargo_counts = remaining_cargoes.sum(-1)    4 .. 7 awaiting_cargo_counts    8 .. 23 remaining_cargoes [warehouse][destination]
//
// individual_done needs the goals of the previous step: an engine-owned snapshot [N][Nt + 1] int32 (the goals, then the episode number EI_EPISODE),
// of its own -- not the reward rows': either attachment works without the other.  A step of another episode than the snapshot's reports 0; every
// reset, restart and import is followed by the snapshot-only form.  An environment whose record says done = 2 keeps rows and snapshot untouched.
// A multi-frame call describes its last frame and reports NaN there (InfoArgs::done_nan): a delivery between the frames cannot be seen from the end state.
//
// Mapping: the tile of attached_tile.hpp; lane j of a group is camera j AND target j.  The camera -> target words go through LDS (view_words); target j's
// Nc camera bits sit in its own row of the mask record (bit_target_row + j (Nc + No + Nt), at most two words) and lane j extracts them itself; an OR
// butterfly over the group turns the lanes' fields into the words whose bit c is is_sensed(c) and whose bit t is is_tracked(t).  Each output of a tile is one
// contiguous stretch of HBM: the rows are put together in LDS and leave as 16-byte pieces, whole waves storing consecutive addresses.
//
// This header holds the arguments and the launch function's declaration; the kernel is info_kernels.hip, a translation unit of its own
// (mate_amd/build.py: lib/kernel_resources_info.json).
#pragma once
#include "attached_tile.hpp"

namespace mate {

constexpr int kInfoCameraColumns = 2, kInfoTargetColumns = 9, kInfoCargoColumns = 24;
enum InfoMode : int32_t { INFO_STEP = 0, INFO_SNAPSHOT = 1, INFO_ON_DEMAND = 2 };

struct InfoArgs {
    const float *scalars;         // [N][8] of the step the rows describe (INFO_STEP only)
    const uint32_t *masks;        // [N][MW] of that step; null (INFO_ON_DEMAND): the three mask columns read NaN
    const double *dyn;            // Ptrs::dyn: the environments' records
    int32_t *snapshot;            // [N][Nt + 1]: the goals the previous launch saw, then its episode number (untouched by INFO_ON_DEMAND)
    double *cam_rows, *tgt_rows, *cargo_rows;      // [N][Nc][2] / [N][Nt][9] / [N][24], 16-byte aligned, any may be null
    int64_t N;
    int32_t mode;
    int32_t done_nan;             // the call ran more than one frame: individual_done reads NaN
    int32_t bit_ct, bit_tr;       // mate_layout.bit_camera_target, bit_target_row
};

// dynamic LDS of a tile: its records, then its target, camera and cargo rows as they leave
__host__ __device__ constexpr int info_rows_lds_bytes(int DW, int Nc, int Nt) {
    return attached_tile_lds_bytes(DW) + kAttachedEnvsPerBlock * (Nt * kInfoTargetColumns + Nc * kInfoCameraColumns + kInfoCargoColumns) * 8;
}

// info_rows_kernel on `blocks` tiles with `lds` bytes of dynamic LDS; returns the launch's error
hipError_t launch_info_rows(unsigned blocks, size_t lds, hipStream_t stream, const Params *params, const InfoArgs &a);

}  // namespace mate
