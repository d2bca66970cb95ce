// trace_rows.hpp -- comm_trace_kernel: the state of mate.RenderCommunication (mate/wrappers/render_communication.py:42-56 of the reference) kept on the device,
// the rules of DESIGN.md 3.21.  Per team an engine-owned uint8 matrix remaining[N][sender][recipient]: how many more frames the arrow of that pair is drawn
// (render_rows.hpp draws it).  ONE launch per stepping call serves both teams, between the agents' launch and the stepping launch -- the wrapper updates before
// env.step --, for every environment that takes a live step in the call (the rule of every launch in that position: not `freeze_done` with EI_DONE != 0, which is
// exactly the environments whose scalar record will not say done = 2; the one-launch step idles every finished environment, so its call passes freeze_done = 1):
//   1  remaining = max(remaining - 1, 0); an environment whose tag is not its episode number starts from zeros and is retagged (the wrapper's reset())
//   2  remaining[s][r] = duration wherever a message s -> r was delivered since the previous step: the team's `delivered` matrix of the agents' launch of THIS
//      call where it ran under a channel (channel_rows.hpp), the team's step_edges > 0 of the routed learner messages where their (tick, episode) tag is the
//      environment's (message_rows.hpp: routed since the last stepping launch), both where both exist
// An environment that idles under a batched restart keeps its bytes and its tag.
//
// Mapping: the tile of attached_tile.hpp, sixteen consecutive environments per 256-thread workgroup.  A team's n n bytes per environment are contiguous, so a tile's
// matrices are ONE run of 16 n n bytes: 16-byte loads and stores where n n is a multiple of 16 (a piece then lies inside one environment, and every tile's run starts
// on a 16-byte boundary of the engine-owned buffers), byte accesses otherwise.  Sixteen lanes first read the environments' record words and tags into LDS flags.
// Offsets are 64-bit, stores plain.  Identical arguments at every call of a flow, no allocation, no wait: capturable in a graph.
#pragma once
#include "attached_tile.hpp"

namespace mate {

struct TraceTeam {
    int32_t n, pad;                   // the team's agents (0: the team has no trace)
    uint8_t *remaining;               // [N][n][n], engine-owned
    int32_t *tags;                    // [N]: the episode number the matrix belongs to (-1: none)
    const int8_t *delivered;          // [N][n][n] of the agents' launch of this call, or NULL
    const int32_t *step_edges;        // [N][n][n] of the routed learner messages, or NULL
    const int32_t *message_tags;      // [N][2] their (tick, episode) tags
};

struct TraceArgs {
    TraceTeam team[2];                // MATE_TEAM_CAMERA, MATE_TEAM_TARGET
    const double *dyn;                // Ptrs::dyn: the environments' records (tick, episode number, done word)
    int64_t N;
    int32_t duration;                 // 1 .. 255
    int32_t freeze_done;              // Ptrs::freeze_done of the call
};

// comm_trace_kernel on `blocks` tiles; returns the launch's error
hipError_t launch_comm_trace(unsigned blocks, hipStream_t stream, const Params *params, const TraceArgs &a);

// trace_plant_kernel on `blocks` tiles: `src` [N][nn] into `dst`, the tags to the episode numbers of the records; returns the launch's error
hipError_t launch_trace_plant(unsigned blocks, hipStream_t stream, const Params *params, const double *dyn, const uint8_t *src, uint8_t *dst, int32_t *tags, int64_t N, int32_t nn);

}  // namespace mate
