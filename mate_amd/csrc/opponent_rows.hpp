// opponent_rows.hpp -- the scripted opponents beyond the Greedy pair, one launch each: HeuristicTargetAgent first, HeuristicCameraAgent below it.
//
// HeuristicTargetAgent (mate/agents/heuristic.py:290-337) as ONE launch
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
// This header holds the arguments and the launch function's declaration only; the kernel and that function are opponent_kernels.hip: not a
// template, so compiled exactly once, in a translation unit of its own (mate_amd/build.py: UNITS).
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

// ---------------------------------------------------------------------------------------------------------------------------------------
// HeuristicCameraAgent (mate/agents/heuristic.py:17-231) as ONE launch, heuristic_camera_kernel, in front of the stepping launch: the camera
// team's joint action where the engine plays that team (mate_engine_set_camera_opponent).  Under mate.group_step camera 0 is the controller:
// every camera sends it its observation and gets its goal back within the step, so the team is one central computation per environment.
//
// Tables (host arrays of the caller, mate_engine_heuristic_camera_tables; mate_amd/heuristic_tables.py builds them):
//   state_mesh [756][3]   state s = a 36 + o: (orientation -180 + 10 o, viewing angle linspace(theta_min, 180, 21)[a], sight range)
//   coord_grid [2952][2]  point g = p 41 + r: polar (linspace(0, Rmax, 41)[r], -180 + 5 p) as Cartesian
//   scores [2952][756]    f64 (17.8 MB, ~14 % non-zero): calculate_scores (:235-287)
// Per environment and step (:168-231), f64, product then add (-ffp-contract=off):
//   sensed       the union over the cameras of the camera_target_view_mask rows the agents act on (the engine's own mask words), listed in
//                insertion order: cameras ascending, within a camera the not yet listed targets ascending.  Locations from the records.
//   in range     of camera c: the listed targets with norm2(target - camera) <= Rmax, in list order
//   nearest      per in-range pair, g = the FIRST minimum over all 2952 points of sqrt(ex ex + ey ey), e = (target - camera) - grid[g].
//                Compared on the squares; where two squares lie within 2^-50 of each other their correctly rounded roots decide, so the
//                result is the reference's argmin of the roots, ties to the lower index, at one root per lane
//   accumulate   scores_c[s] += scores[g][s] in list order; bit t of bits_c[s] where scores[g][s] > 0
//   32 permutations of the cameras (tape, or Philox: below); per permutation, in its order, from cur = 0, total = 0, cost = 0:
//                i = first maximum over s of scores_c[s] + popcount(bits_c[s] & ~cur)
//                cost += max(|mesh[i].orientation - phi_c| / rotation_step, |mesh[i].angle - theta_c| / zooming_step)   (plain differences)
//                cur |= bits_c[i]; total += scores_c[i];   after the last camera total += popcount(cur)
//   winner       the maximum of (total, -cost, permutation, indices) as tuples: equal totals and costs go to the lexicographically larger
//                permutation (equal permutations have equal indices)
//   goal         camera c: mesh[i_c] of the winner iff c has an in-range target
//   act (:59-95) with a goal clip((normalize_angle(goal_o - phi), goal_a - theta), +-(rotation_step, zooming_step)); without one a
//                Bernoulli(0.1) uniform u: u > 0.9 a uniform sample of the action box, else the previous action.  prev_action (the agent's only
//                memory) is (0, 0) at the team's first acting call of an episode (the tag `episode` below, as for the Greedy teams).
//                The fallback branch of a non-controller (:73-78) never finds a target (a camera that senses one has it in range) and draws nothing.
// Draws: Philox (seed, global environment index, tick) on streams of their own --
//   S_HCAM_PERM  sub = 2 k + h: sixteen 16-bit words w_0..w_15 of permutation k (h = 0: w_0..w_7, low half of .x first).  Fisher-Yates from
//                the identity: for i = Nc - 1 down to 1, j = (w_{Nc-1-i} (i + 1)) >> 16, swap(a[i], a[j])   (bias below 2^-12 per draw)
//   S_HCAM_ACT   sub = c: .y the Bernoulli uniform, .z / .w the two sample uniforms (32-bit, as the Greedy cameras' draws)
// or the tapes: permutations [N][32][Nc] int8 (entries are clamped to [0, Nc)), PolicyTape::cam_binom_u / cam_sample_u.
//
// Mapping: one 256-thread workgroup per environment, dynamic LDS max(47 232, Nc 7560) bytes used twice --
//   0  32 threads draw (or read) the permutations into LDS; the mesh's two columns (36 orientations, 21 angles) and coord_grid (47 KB,
//      eleven or twelve 16-byte loads per thread in flight at once) are staged; thread c < Nc lists camera c's in-range targets
//   1  every in-range pair is one wave's job, its 64 lanes split the 2952 points, a wave argmin leaves g
//   2  the same bytes become scores_c[Nc][756] f64 + bits_c[Nc][756] u16; thread tid holds states tid, tid + 256, tid + 512 and adds the
//      6 KB rows scores[g][.] of HBM in list order, three independent coalesced loads per row in flight
//   3  each wave takes eight permutations AT ONCE, eight lanes each: a pick is 95 elements per lane and a three-step argmax within the
//      group that keeps the lowest index among equals (a camera without in-range targets picks state 0 without the pass: its scores
//      and bits are zeros).  The chain of picks is serial per permutation and bound by latency, not issue: eight chains per wave, short
//      reductions and unrolled loads took a graph-replayed step of MATE-4v8-9 x 4096 from 820 to 467 us
//   4  thread 0 picks the winner, threads c < Nc write goal, action and prev_action
// An environment idling under a batched restart (done != 0 with freeze_done) is skipped: its rows and its prev_action stay.
constexpr int kHcStates = 756, kHcPoints = 2952, kHcPermutations = 32, kHcMaxAgents = 16;
enum HeuristicCameraStream : uint32_t { S_HCAM_PERM = 20, S_HCAM_ACT = 21 };
__host__ __device__ constexpr size_t heuristic_camera_lds_bytes(int Nc) {
    return (size_t)kHcPoints * 16 > (size_t)Nc * kHcStates * 10 ? (size_t)kHcPoints * 16 : (((size_t)Nc * kHcStates * 10 + 15) & ~(size_t)15);
}

struct HeuristicCameraArgs {
    const double *mesh, *grid, *scores;      // the three tables on the device
    const uint32_t *masks;                   // [N][MW]: the engine's own mask words, the view the agents act on
    double *action;                          // [N][Nc][2], engine-owned: the camera team's joint action of the stepping launch
    double *prev_action;                     // [N][Nc][2]
    double *goals;                           // [N][Nc][2], NaN where none
    int32_t *goal_index;                     // [N][Nc], -1 where none
    int32_t *episode;                        // [N]: the episode whose first call has run the agents' reset
    const double *binom_u, *sample_u;        // PolicyTape::cam_binom_u [N][Nc] / cam_sample_u [N][Nc][2], or NULL: Philox
    const int8_t *permutations;              // [N][32][Nc] recorded permutations, or NULL: Philox
    int8_t *record;                          // [N][32][Nc]: receives the permutations used, or NULL (a wave-uniform branch)
    int32_t freeze_done;                     // Ptrs::freeze_done of the call
};

// heuristic_camera_kernel, one workgroup per environment with heuristic_camera_lds_bytes(Nc) of dynamic LDS; returns the launch's error
hipError_t launch_heuristic_camera(unsigned blocks, size_t lds, hipStream_t stream, const Params *params, const Ptrs &g, const HeuristicCameraArgs &a);
const void *heuristic_camera_function();      // (for hipFuncSetAttribute: the dynamic LDS passes 64 KB from nine cameras on)

}  // namespace mate
