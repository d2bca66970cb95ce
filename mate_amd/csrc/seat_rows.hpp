// seat_rows.hpp -- a learner seat among on-device teammates: the reference's SingleCamera / SingleTarget wrappers (mate/wrappers/single_team.py:310-470,
// SingleTeamSingleAgent) over Greedy teammates, as two launches around the stepping launch -- greedy_seat_kernel in the place of the stand-alone agents'
// launch of the two-launch form (greedy_policy_kernel: one wave per environment, four per workgroup) and seat_rows_kernel behind the restart epilogue.
// The agents are greedy_policy_body itself, instantiated with the Seat policy below; nothing of the agents is restated here.
//
// Semantics.  The learner plays ONE slot `z` of its team, the seat; the other n - 1 slots are the team's Greedy agents with their TRUE indices (agent.reset reads
// the index from the observation row), the opposing team is whatever the call's opponent plan makes of it.  Around the seat:
//   camera teammates (greedy.py:158-226)   the send loop skips only the sender's own index, so every teammate DOES send its one 'state' message to the seat and draws
//                 that pair's randint(6, 50) delay; the seat never answers, so it never becomes anybody's neighbour, no teammate's later message to it has content,
//                 and none is sent or drawn.  The seat itself sends nothing, draws nothing, keeps no memory another agent reads.
//   target teammates (greedy.py:331-365)   broadcast to every slot, the seat included (no effect there); the seat broadcasts nothing: it is never among the
//                 senders, and its non_empty_warehouses does not exist.
//   act           slot z runs no agent: the lane decodes the learner's action exactly as a caller's row is decoded (f32 / f64 pair, or a grid index with the
//                 team's *_DISCRETE bit: load_caller_actions) and writes it into the team's joint-action row (PolicyPtrs::cam_act / tgt_act), so the stepping launch
//                 and mate_engine_policy_actions see the final rows.  prev_action(z) is not touched.
// The learner's own send_messages / receive_messages are not provided: reference-format messages authored by a learner were never on the device.
//
// The seat of an episode is a pure function of (mode, seed, global environment index, episode, team), so every launch evaluates it for itself (seat_of_episode):
//   SEAT_FIXED    a constant (the wrapper's index = num_teammates - 1 with shuffle_entities off)
//   SEAT_DRAW     (uint64(philox(seed, env_global, episode, S_SEAT, team).x) * n) >> 32: np_random.randint(n) drawn anew at every reset()
//   SEAT_TAPE     a caller-owned [N] int32 read at every launch; a value outside [0, n) falls back to SEAT_DRAW
//
// greedy_seat_kernel: both teams' agents act (but the team `q.caller_team` names: an opposing team played by other launches).  It stores seat_acted[N], the seat
// whose action the launch consumed, and live[N] = 1; an environment the launch skips (finished, waiting for the batched restart) keeps seat_acted and reads live = 0.
// seat_rows_kernel: the LAST launch of a seat call.  A workgroup per tile of 16 environments; it gathers row seat(env) of the team's output observations
// ([N][n][D]) into seat_obs[N][D] and writes seat_index[N], the seat of the episode the row belongs to (after an immediate restart: the new episode's).  An
// environment that idled through the whole call (live = 0 and still finished) keeps both.  The tile's destination is one contiguous run of 16 D elements: 16-byte
// stores of gathered elements wherever the four (two) elements' environments are all written, element stores at the rims.
#pragma once
#include "policy_kernels.hpp"

namespace mate {

enum SeatStream : uint32_t { S_SEAT = 27 };               // behind S_CHAN_DROP = 26
enum SeatMode : int32_t { SEAT_FIXED = 0, SEAT_DRAW = 1, SEAT_TAPE = 2 };

struct SeatSpec {
    int32_t team, mode, fixed, n;     // MATE_TEAM_*; SEAT_*; the constant of SEAT_FIXED; the team's agents
    const int32_t *tape;              // [N] (SEAT_TAPE)
};

// The DRAW formula, host and device: word .x of the Philox block scaled to [0, n)
__host__ __device__ constexpr int seat_from_word(uint32_t x, int n) { return (int)(((uint64_t)x * (uint64_t)n) >> 32); }

__device__ __forceinline__ int seat_of_episode(const Params &p, const SeatSpec &s, int64_t env, int32_t episode) {
    if (s.mode == SEAT_FIXED) return s.fixed;
    if (s.mode == SEAT_TAPE) { const int v = s.tape[env]; if (v >= 0 && v < s.n) return v; }
    const U4 r = philox(p.seed_lo, p.seed_hi, p.first_env + (uint32_t)env, (uint32_t)episode, S_SEAT, (uint32_t)s.team);
    return seat_from_word(r.x, s.n);
}

struct SeatArgs {
    SeatSpec spec;
    int32_t *acted;                   // [N] the seat whose action the launch consumed
    int32_t *live;                    // [N] 1: the launch ran the environment, 0: it skipped it
};

struct SeatRowsArgs {
    SeatSpec spec;
    const void *rows;                 // [N][n][D] the team's output observations of the call
    void *seat_obs;                   // [N][D]
    int32_t *seat_index;              // [N]
    const int32_t *live;              // [N] greedy_seat_kernel's of this call, or NULL (on demand: every environment is written)
    int32_t D;
};

constexpr int kSeatRowsEnvs = 16;     // environments per workgroup of seat_rows_kernel

// The Seat policy of greedy_policy_body (see NoSeat there) of one environment: slot `z` of team `team` is the learner's.
struct LiveSeat {
    static constexpr bool kLive = true;
    const Params &p;
    const Ptrs &g;                    // the call's record pointers: the seat team's action pointer, encoding and grid
    const PolicyPtrs &q;
    int team, z;
    int64_t env;

    __device__ __forceinline__ bool camera(int c) const { return team == 0 && c == z; }
    __device__ __forceinline__ bool target(int t) const { return team != 0 && t == z; }
    __device__ __forceinline__ void act_camera(int c) const {
        double da, dz;
        if (g.act_discrete & 1) {
            int idx = reinterpret_cast<const int32_t *>(g.cam_act)[env];
            idx = idx < 0 ? 0 : (idx >= g.n_cam_grid ? g.n_cam_grid - 1 : idx);
            const double2 gxy = g.cam_grid[idx];
            da = p.rot * gxy.x; dz = p.zoom * gxy.y;
        } else if (g.act_f64 & 1) {
            const double *a = reinterpret_cast<const double *>(g.cam_act) + env * 2;
            da = a[0]; dz = a[1];
        } else {
            const float2 a = reinterpret_cast<const float2 *>(g.cam_act)[env];
            da = (double)a.x; dz = (double)a.y;
        }
        q.cam_act[(env * p.Nc + c) * 2] = da; q.cam_act[(env * p.Nc + c) * 2 + 1] = dz;
    }
    __device__ __forceinline__ void act_target(int t, uint64_t capword) const {
        double ax, ay;
        if (g.act_discrete & 2) {
            int idx = reinterpret_cast<const int32_t *>(g.tgt_act)[env];
            idx = idx < 0 ? 0 : (idx >= g.n_tgt_grid ? g.n_tgt_grid - 1 : idx);
            const double2 gxy = g.tgt_grid[idx];
            const double high = ((capword >> t) & 1ull) ? p.tgt_step * 0.5 : p.tgt_step;   // loaded targets halve their step
            ax = high * gxy.x; ay = high * gxy.y;
        } else if (g.act_f64 & 2) {
            const double *a = reinterpret_cast<const double *>(g.tgt_act) + env * 2;
            ax = a[0]; ay = a[1];
        } else {
            const float2 a = reinterpret_cast<const float2 *>(g.tgt_act)[env];
            ax = (double)a.x; ay = (double)a.y;
        }
        q.tgt_act[(env * p.Nt + t) * 2] = ax; q.tgt_act[(env * p.Nt + t) * 2 + 1] = ay;
    }
};

// greedy_seat_kernel<float / double observations> on `blocks` workgroups of four environments with `lds` bytes (4 PolicyPtrs::lds_bytes); returns the launch's error
hipError_t launch_greedy_seat(bool obs_f64, unsigned blocks, size_t lds, hipStream_t stream, const Params *params, const Ptrs &g, const PolicyPtrs &q, const SeatArgs &a);
const void *greedy_seat_function(bool obs_f64);      // (for hipFuncSetAttribute)
// seat_rows_kernel<float / double rows> on `blocks` workgroups of kSeatRowsEnvs environments
hipError_t launch_seat_rows(bool obs_f64, unsigned blocks, hipStream_t stream, const Params *params, const Ptrs &g, const SeatRowsArgs &a);

}  // namespace mate
