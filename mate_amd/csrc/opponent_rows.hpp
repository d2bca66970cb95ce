// opponent_rows.hpp -- the scripted opponents beyond the Greedy pair: HeuristicTargetAgent (mate/agents/heuristic.py:290-337) as ONE launch
// between the agents' launch and the stepping launch of the two-launch form (step_with_policies, mate_engine.hip).  The reference's agent is
// GreedyTargetAgent.act followed by a post-processing of the returned action -- no draw, no memory, no message of its own -- so the launch is a
// pass over the Greedy agents' joint action: out of place, q.tgt_act keeps the Greedy action, the final action goes to an engine-owned
// [N][Nt][2] f64 buffer the stepping launch reads as the target team's.
//
// Per target, heuristic.py:298-337 with the reference's operations in the reference's order:
//   sensed[c]    the target's target_camera_view_mask bit (the flag column of the camera blocks of its PLAIN observation row) of the view the
//                agents act on: bit_target_row + t * NJ + c of the engine's own mask words
//   candidate    norm(target - camera) <= 1.2 sight_range  and  normalize_angle(atan2_deg(target - camera) - orientation) <= 1.2 half
//                -- the SIGNED difference, as the reference compares it (:308-311, no abs): a target far to the clockwise side of a camera it
//                senses is a candidate.  Reproduced, not corrected.
//   centre       camera + (sight_range / (1 + sin_deg(min(half, 90)))) (cos phi, sin phi), inner_radius = sight_range - that norm   (:313-318)
//   choice       the first minimum, in camera order, of norm(target - centre) / inner_radius                                       (:322-325)
//   drift        target - centre, scaled to step_size * noise_scale where longer                                                   (:327-330)
//   action       clip(action + drift, +-step_size) where dot(action, drift) >= 0, else unchanged                                  (:332-335)
// phi, theta and the sight range come from the records (the reference decodes them from the observation's (Rs cos phi, Rs sin phi) pair,
// agents/utils.py:206-216: the same values up to rounding -- the parity bar is a tolerance, as for the Greedy agents).
//
// An environment the agents' launch skips (done != 0 under a batched restart, Ptrs::freeze_done) is skipped here: its final row is its Greedy
// row.  A scenario without cameras makes the launch a plain copy.
//
// Mapping: the tile of attached_tile.hpp, lane j of a group is target j; the camera locations of the static records are staged next to the
// dynamic records; each target lane reads the (at most two) mask words that hold its row's camera bits.  f64 throughout, product then add
// (-ffp-contract=off); fused where the Greedy agents' code fuses (norm2).
//
// This header holds the arguments and the launch function's declaration only; the kernel and that function are opponent_kernels.inc: not a
// template, so compiled exactly once -- in a translation unit of its own (opponent_kernels.hip) under mate_amd/build.py, inside mate_engine.hip
// in the single-unit build, as shape_group.inc is.
#pragma once
#include "attached_tile.hpp"
#include "policy_kernels.hpp"

namespace mate {

struct DriftArgs {
    const double *greedy;         // [N][Nt][2]: PolicyPtrs::tgt_act as the agents' launch of this call left it
    double *final_act;            // [N][Nt][2], engine-owned: the target team's joint action of the stepping launch
    const uint32_t *masks;        // [N][MW]: the engine's own mask words, the view the agents acted on
    double noise_scale;           // PolicyPtrs::noise_scale (0.5, greedy.py:236)
    int32_t bit_tr;               // mate_layout.bit_target_row
    int32_t freeze_done;          // Ptrs::freeze_done of the agents' launch
};

// heuristic_drift_kernel on `blocks` tiles with `lds` bytes of staged records (attached_tile_lds_bytes); returns the launch's error
hipError_t launch_heuristic_drift(unsigned blocks, size_t lds, hipStream_t stream, const Params *params, const Ptrs &g, const DriftArgs &a);

}  // namespace mate
