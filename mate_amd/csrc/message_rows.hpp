// message_rows.hpp -- the learner's own messages through the team's channel: the environment's send_messages / receive_messages and the communication-edge counts
// of `info` (mate/environment.py:836-892, 634-668, 823-830, route_messages 1249-1269) under the channel wrappers (mate/wrappers/message_filter.py:39-50 and its three
// subclasses), as ONE launch on demand, message_rows_kernel: fixed-width payloads the learner wrote on the device go sender -> recipient under the channel
// mate_engine_set_channel configured for the team, by channel_verdict itself (channel_rows.hpp: included, not restated), from the positions of the current records.
//
// Semantics.  A message is `width` numbers of the observation type from sender s to recipient r of one team; one launch routes at most one message per ordered
// pair and team.  The payload is [N][n][width] (one content per sender, to everyone it addresses) or, `pairwise`, [N][n][n][width] ([sender][recipient]).  Who is
// addressed: a caller-written [N][n][n] uint8 `address`, [sender][recipient], read at every launch; NULL: broadcast -- to every slot of the team, the sender's own
// included (route_messages), an edge like any other with distance 0.  A sent message arrives iff channel_verdict says so for the team's channel; with no channel
// set everything arrives.  Distances: norm2 over the static record for cameras, the dynamic record for targets -- the positions the observation rows of this
// moment show.  The mask byte is the channel's own mask.
//
// Draws: one uniform per (team, round, sender, recipient), only where the team's rate is > 0 and the message was sent: a tape ([N][n][n] f64) or Philox
// (seed, global environment index, tick, S_MSG_DROP, round << 12 | team << 8 | sender << 4 | recipient), word .x as a 32-bit uniform like the agents' channel --
// independent of first_env_index and of sharding.  `round` (0..15) is the call's: the reference's agents talk twice per step, a learner may route several times
// between two steps.  A record buffer receives the uniform each verdict used, NaN where none was drawn.
//
// Outputs, engine-owned, per team:
//   inbox [N][n recipient][n sender][width]   the delivered content, zeros where nothing was sent or nothing arrived (what ActionWithMessage.reset hands out).  The
//                 launch writes the whole block: no memset.  Recipient-major: agent r's input is one contiguous [n][width] run.
//   sent, delivered   int8 [N][n][n], [sender][recipient], of this call
//   step_edges    int32 [N][n][n]: deliveries since the last stepping launch (the reference's *_communication_edges, which step() reports and clears)
//   total_edges   int32 [N][n][n]: the steps of the episode before this one (the reference's *_total_communication_edges as step() left them)
//   agent_edges   int32 [N][n][2]: out_ / in_communication_edges of `info`, the row and column sums of step_edges
// Tags: a (tick, episode) pair per team and environment makes the counts a pure function of what the launch sees -- a tick other than the tag's folds step_edges
// into total_edges and zeroes it, an episode other than the tag's zeroes both.  Nothing is attached to the stepping flows.  An environment whose episode is
// over (EI_DONE != 0: finished, waiting for a batched restart or for the caller's reset) is skipped and keeps every row, the inbox included.
//
// Mapping: one wave per environment, four per workgroup, as greedy_channel_kernel -- an environment's inbox block is ONE contiguous run of n n width elements, so
// the wave's 64 lanes store whole 1 KB lines of it back to back, and the verdict ballots it needs stay in the wave (no workgroup barrier).  Verdicts one pair per
// lane, 64 per round (up to four at 16 x 16), balloted into delivered words in LDS; the edge bytes are staged there and leave as 4-byte stores where n n is a
// multiple of four, as byte stores else.  Payload: 16-byte loads and 16-byte non-temporal stores where width sizeof(ObsT) is a multiple of 16 (the host checks the
// buffers' alignment), an element path else; stores are coalesced along [sender][width].  LDS per wave: 4 delivered words, 2 x 256 edge bytes, 256 counts.
#pragma once
#include "channel_rows.hpp"

namespace mate {

enum MessageStream : uint32_t { S_MSG_DROP = 28 };        // behind S_SEAT = 27

constexpr int kMessageRounds = 16;                        // `round` lies in [0, kMessageRounds)
constexpr int kMessagePairs = 256;                        // 16 x 16 agents at most

struct MessageTeam {
    int32_t on, n, width, pairwise;   // the launch routes the team; its agents; numbers per message; the payload is [N][n][n][width]
    int32_t set, disabled;            // the team's channel (ChannelTeam's four settings and its mask)
    double limit, rate;
    const uint8_t *mask;              // [N][n][n] or NULL
    const uint8_t *address;           // [N][n][n] or NULL (broadcast)
    const void *payload;              // [N][n][width] / [N][n][n][width] ObsT
    void *inbox;                      // [N][n][n][width] ObsT, [recipient][sender]
    const double *tape_u;             // [N][n][n] or NULL (Philox)
    double *record_u;                 // [N][n][n] or NULL
    int8_t *sent, *delivered;         // [N][n][n]
    int32_t *step_edges, *total_edges, *agent_edges;      // [N][n][n], [N][n][n], [N][n][2]
    int32_t *tags;                    // [N][2]: the tick and the episode the counts belong to
};

struct MessageArgs {
    MessageTeam team[2];              // MATE_TEAM_CAMERA, MATE_TEAM_TARGET
    int32_t round;
};

// The Philox sub-stream of one draw (host and device)
__host__ __device__ constexpr uint32_t message_draw_key(int round, int team, int s, int r) { return (uint32_t)(round << 12 | team << 8 | s << 4 | r); }

// message_rows_kernel<float / double payloads> on `blocks` workgroups of four environments; returns the launch's error
hipError_t launch_message_rows(bool obs_f64, unsigned blocks, hipStream_t stream, const Params *params, const Ptrs &g, const MessageArgs &a);

}  // namespace mate
