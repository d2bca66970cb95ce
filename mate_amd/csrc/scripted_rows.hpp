// scripted_rows.hpp -- the scripted agent families beyond the Greedy and Heuristic pairs, and the per-episode MIXTURE over all of them, as ONE launch
// (OpponentPlan::team[].scripted, engine_host.h): scripted_opponent_kernel, behind the agents' launch, the Heuristic cameras' launch and the drift launch,
// ahead of the stepping launch.  Per environment and per team the engine plays it (1) runs the team's reset, the mixture draw included, at the team's first
// acting call of an episode, (2) computes the Naive or Random agents' action where the episode's choice asks for it, (3) writes the team's FINAL joint action --
// one of five sources -- into an engine-owned [N][n][2] f64 buffer the stepping launch reads, (4) fills the record of the draws it used.
//
// MixtureCameraAgent / MixtureTargetAgent (mate/agents/mixture.py:101-109).  spawn() seeds every agent of a team alike, so the whole TEAM plays one candidate
// per episode: at the team's first acting call of an episode (the tag `episode`, as for the Greedy teams and heuristic_camera_kernel)
//   k = searchsorted(cum, u, side='right'), cum = cumsum(w / sum w) over the candidates with positive weight in the order given   (RandomState.choice(p=))
// i.e. the first k with u < cum[k] (the last candidate where rounding leaves cum short of u); `choice` holds the candidate's KIND for the episode.  Only the
// chosen candidate's reset runs (mixture.py:109).  The host passes cum with the zero-weight candidates removed.
//
// NaiveCameraAgent (mate/agents/naive.py:18-29): action = (0.0 + 0.4 u) (rotation_step, zooming_step); one uniform per camera and frame, no memory.
//
// NaiveTargetAgent (naive.py:32-105); memory per target goal (0..3), inc (+-1), prev_location, prev_noise:
//   reset    prev_noise = 0.5 sample(); goal = choice(4); inc = choice([+1, -1]); prev_location = location                              (:56-68)
//   arrival  norm(location - WAREHOUSES[goal]) <= 0.9 WAREHOUSE_RADIUS: goal = (goal + inc) mod 4 -- once where the target carries a goal
//            (goal_bits.any(): a goal with a positive weight) or every warehouse is empty to its knowledge, else until a warehouse it does not
//            know to be empty is reached                                                                                                (:79-86)
//   action   goal - location cut to step_size; prob = 0.05 where norm(location - prev_location) > 0.2 step_size, else 0.75; binomial(1, prob)
//            resamples noise = 0.5 sample() or keeps prev_noise; clip(action + noise, +-step_size)                                      (:88-105)
// goal_bits and empty_bits are the target's own (TI_GW of the records: the columns of its PLAIN row).  The noise rule is GreedyTargetAgent's line for
// line (greedy.py:319-328; greedy_policy_body in policy_kernels.hpp), with the same mapping of a uniform to binomial(1, prob): prob <= 0.5 draws 1 where
// u > 1 - prob, else where u <= prob.  It is restated in scripted_kernels.hip, not shared as a function: policy_kernels.hpp is part of every fused kernel's
// source, which this launch leaves as it is.
//
// RandomCameraAgent / RandomTargetAgent (mate/agents/random.py): a new action_space.sample() (low + (high - low) u) at the agent's own acting calls
// number 0, frame_skip, 2 frame_skip, ... of an episode, else the previous action.  Memory: prev_action and the call counter (one per team: its agents act together).
//
// EXTERNAL: rows the caller wrote into an engine-owned [N][n][2] f64 buffer before the call (a learned population member evaluated on the host side of
// the batch); the launch copies the rows of the environments that drew it.
//
// An environment the agents' launch skips (done != 0 with freeze_done) is skipped: memory, choice and final row stay; its record entries read NaN.
//
// Draws: Philox (seed, global environment index, tick or episode) on streams of their own, 32-bit uniforms as the Greedy agents' --
//   S_SCR_CHOICE      (episode, sub = team): u = u53(.x, .y), the mixture draw
//   S_SCR_CAMERA      (tick, sub = c): .x -> camera_u[0] (Naive's u, Random's first), .y -> camera_u[1]
//   S_SCR_TARGET      (tick, sub = t): .x the binomial u, .y / .z the two sample uniforms (Random uses the latter two)
//   S_SCR_TARGET_RESET(episode, sub = t): .x / .y the sample uniforms of prev_noise, .z >> 30 the goal, .w >> 31 ? -1 : +1 the inc
// or a tape (ScriptedDraws, any member NULL: Philox for that member): camera_u [N][Nc][2], target_u [N][Nt][3], target_reset [N][Nt][4] (u0, u1, goal, inc
// as doubles), choice [2][N] int32 KINDS (-1: draw; a kind outside the team's mixture: draw).  The record has the same shapes and receives what the launch
// used, NaN where nothing was drawn; its choice rows receive the kind every live team holds (-1: no mixture).
//
// Mapping: the tile of attached_tile.hpp -- sixteen environments per 256-thread workgroup, lane j of a group is camera j AND target j; the dynamic records
// are staged with stage_records.  Every row of a tile is contiguous: a lane stores its agent's (x, y) as one 16-byte piece, consecutive lanes on consecutive
// addresses.  Lanes beyond the batch take part in the staging barrier only: no load, shuffle or store.  f64 throughout, product then add (-ffp-contract=off);
// fused where the Greedy agents' code fuses (norm2).
#pragma once
#include "attached_tile.hpp"

namespace mate {

enum ScriptedKind : int32_t { SCRIPTED_GREEDY = 0, SCRIPTED_HEURISTIC = 1, SCRIPTED_NAIVE = 2, SCRIPTED_RANDOM = 3, SCRIPTED_EXTERNAL = 4, kScriptedKinds = 5 };
enum ScriptedTeamIndex : int { SCRIPTED_CAMERAS = 0, SCRIPTED_TARGETS = 1 };      // MATE_TEAM_CAMERA / MATE_TEAM_TARGET of the C ABI
enum ScriptedStream : uint32_t { S_SCR_CHOICE = 22, S_SCR_CAMERA = 23, S_SCR_TARGET = 24, S_SCR_TARGET_RESET = 25 };

struct ScriptedDraws {                // a tape (read) or a record (written); any member may be NULL
    double *camera_u;                 // [N][Nc][2]
    double *target_u;                 // [N][Nt][3]
    double *target_reset;             // [N][Nt][4]
    int32_t *choice;                  // [2][N]
};

struct ScriptedTeam {                 // one team's mixture; on == 0: the launch leaves the team alone
    int32_t on, count, frame_skip, n; // installed; candidates with positive weight; RandomAgent.frame_skip; agents of the team
    int32_t kinds[kScriptedKinds];    // ... their kinds in the order given
    double cum[kScriptedKinds];       // ... cumsum(w / sum w)
    const double *rows[kScriptedKinds];  // [N][n][2] per kind: the Greedy row, the Heuristic row, NULL (Naive, Random: the launch's own), the external row
    double *final_act;                // [N][n][2]: the team's joint action of the stepping launch
    int32_t *episode, *choice, *counter;      // [N] each: the episode whose first call has reset the team; the kind it holds; the Random agents' acting calls
    double *prev_action;              // [N][n][2]: the Random agents'
    int32_t *goal, *inc;              // [N][Nt] each: the Naive targets' (NULL for the cameras)
    double *prev_location, *prev_noise;       // [N][Nt][2] each
};

struct ScriptedArgs {
    ScriptedTeam team[2];             // MATE_TEAM_CAMERA, MATE_TEAM_TARGET
    ScriptedDraws tape, record;
    int32_t freeze_done;              // Ptrs::freeze_done of the agents' launch
};

// scripted_opponent_kernel on `blocks` tiles with `lds` bytes of staged records (attached_tile_lds_bytes); returns the launch's error
hipError_t launch_scripted_opponents(unsigned blocks, size_t lds, hipStream_t stream, const Params *params, const Ptrs &g, const ScriptedArgs &a);

}  // namespace mate
