// episode_rows.hpp -- per-episode metric records: what the reference's example trainers report at every episode's end (examples/utils/callbacks.py:
// MetricCollector takes the mean over the agents of each learner step's infos, CustomMetricCallback.on_episode_end reduces each key over the episode's
// steps -- `mean`, `last`, and the `episode_<key>` sums of the keys that end in `reward`), kept on the device behind every stepping flow.  Not on the
// step path: ONE launch of its own (mate_engine_enable_episode_records) behind the reward launch, whose rows it reads, and ahead
// of the restart, so that the records of the environment still say which episode has ended and how long it was.
//
// A learner step of an environment is one frame of the call's scalar records [K][N][8] whose record does not say done = 2.  (A fragment form -- the whole
// fragment of a FrameSkip launch as ONE step, read from the fragment launch's outputs -- is NOT here: see DESIGN.md section 3.12.)
// Per environment the running sums of the learner steps live in an engine-owned table [N][kEpisodeWords] f64 across launches:
//   tag | steps | frames | sum raw reward | sum normalised reward | sum learner reward | sum coverage_rate | sum real_coverage_rate | sum num_tracked
// `tag` is the engine's episode number (EI_EPISODE of the environment's record) the sums belong to: a launch that finds another number there -- every reset,
// restart and import advances or replaces it -- starts from zero; NaN (the table's cleared state, 0xff bytes) equals no number.  A step that says done = 1
// appends one record of kEpisodeColumns doubles to the caller's ring and leaves the sums cleared:
//    0 env   1 episode   2 steps   3 frames   4 length (EI_EPSTEP)   5 episode_raw_reward   6 episode_normalized_raw_reward   7 episode_reward
//    8 raw_reward = [5] / steps   9 normalized_raw_reward = [6] / steps   10 coverage_rate   11 real_coverage_rate (sums / steps)
//   12 mean_transport_rate   13 num_delivered_cargoes (of the last step)   14 num_tracked (sum / steps)   15 team
// Every sum is f64 in step order, product then add (-ffp-contract=off):
//   team reward       scalar column 0 (cameras) or 1 (targets); normalised: column 7, negated for the cameras
//   learner reward    the agent-order sum of the step's reward row: the attached reward rows of the team (one-frame calls, overwrite mode), else the
//                     team reward once per agent; NaN where rows exist but do not describe every step (accumulate mode, a multi-frame call, a
//                     fragment's shaped rows)
//   num_tracked       cameras, and only where the call brought masks (NaN otherwise): popcount of the camera -> target bits / Nc per frame
//
// Mapping: the tile of attached_tile.hpp -- sixteen environments per 256-thread workgroup, a group of 16 lanes each -- and not a lane per environment:
// a lane per environment would read its 32-byte scalar records 32 bytes apart per lane but its sums (72 bytes) and mask words (MW words) with a
// stride per lane, and store its 128-byte record as eight 16-byte pieces, each a line of its own per lane.  In the tile lane j of a group loads word j
// of the sums and of the mask words and stores column j of the record: every access of a group is one contiguous stretch, a tile's sums are 1152
// contiguous bytes, a record is ONE 128-byte line written whole by one store instruction.  The frame walk is fragment_rows_kernel's: all sixteen lanes read the
// frame's record (one address) and carry the same sums; the popcount and the reward row are summed over the group by shuffles, so there is no LDS
// and no barrier, and a launch of N / 16 workgroups of four waves has the occupancy of the other attached launches.
//
// Append: the groups of a wave whose environment finishes take consecutive record numbers through ONE atomic add per wave on the caller's 64-bit counter
// (ballot of the groups' first lanes, the lowest of them adds the popcount, its result is broadcast, a group's rank is the popcount of the lower
// groups); record n goes to slot n % capacity.  Two records of ONE launch can meet in a slot only where capacity < N (an environment appends at most one
// per launch): such a ring is served by the serial form, one workgroup that walks the tiles and appends group by group between barriers, the
// counter in LDS -- correct for any capacity >= 1, and as slow as that sounds.
//
// This header holds the arguments and the launch function's declaration; the kernel is episode_kernels.hip, a translation unit of its own
// (mate_amd/build.py: lib/kernel_resources_episodes.json).
#pragma once
#include "attached_tile.hpp"

namespace mate {

constexpr int kEpisodeColumns = 16, kEpisodeWords = 9;
enum EpisodeWord : int { EW_TAG = 0, EW_STEPS, EW_FRAMES, EW_RAW, EW_NORM, EW_REWARD, EW_COVERAGE, EW_REAL, EW_TRACKED };

struct EpisodeArgs {
    const float *scalars;         // [K][N][8] of the call
    const uint32_t *masks;        // [K][N][MW] of the call, or null (num_tracked reads NaN)
    const void *rows;             // the team's attached reward rows [N][A] of this (one-frame) call, or null
    const double *dyn;            // Ptrs::dyn: the environments' records (episode number, episode step count)
    double *sums;                 // [N][kEpisodeWords], engine-owned
    double *records;              // [capacity][kEpisodeColumns], the caller's ring
    unsigned long long *count;    // records ever appended, the caller's
    int64_t capacity, N;
    int32_t K, team, A;
    int32_t rows_f64;             // the type of `rows`
    int32_t reward_nan;           // the learner's reward rows exist but not for every step of this call: column 7 reads NaN
    int32_t serial;               // 1: the one-workgroup form (capacity < N)
    int32_t bit_ct;               // mate_layout.bit_camera_target
};

// episode_rows_kernel on `blocks` tiles (1 with a.serial); returns the launch's error
hipError_t launch_episode_rows(unsigned blocks, hipStream_t stream, const Params *params, const EpisodeArgs &a);

}  // namespace mate
