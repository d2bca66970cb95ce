// channel_rows.hpp -- communication channels for the scripted agents' messages: the reference's NoCommunication, RandomMessageDropout,
// RestrictedCommunicationRange and the generic MessageFilter (mate/wrappers/) as ONE launch, greedy_channel_kernel, in the place of the stand-alone
// agents' launch of the two-launch form (greedy_policy_kernel: one wave per environment, four per workgroup).  The agents are greedy_policy_body
// itself, instantiated with the Channel policy below; nothing of the agents is restated here.
//
// Semantics (MessageFilter.send_messages, message_filter.py:39-50, over route_messages, environment.py:1249-1269).  A channel belongs to a TEAM and
// decides per step and per routed message sender -> recipient whether it arrives: only where ALL of
//   disabled      NoCommunication(team): nothing arrives
//   range_limit   norm2(recipient - sender) <= limit (restricted_communication_range.py:19-25; `<=`; the positions the agents act on in this call:
//                 the static record's for the cameras, the dynamic record's for the targets; limit < 0: no limit)
//   dropout_rate  dropped iff binomial(1, rate) != 0 (random_message_dropout.py:25-28), with the project's rule for every binomial(1, p) of a uniform u:
//                 1 iff u > 1 - p where p <= 0.5, else iff u <= p.  Rate 0 keeps everything, rate 1 drops everything, by that rule.
//   mask          a caller-written [N][n][n] uint8 buffer, [sender][recipient], non-zero = deliver, read at every launch (a MessageFilter with any function)
// hold (channel_verdict).  What a dropped message changes is what the reference's agents do when receive_responses never sees it; the sender does not know:
//   Greedy cameras (greedy.py:158-226)   the sender's communication_delay is redrawn and message2send cleared as if the message had gone out; only a
//                 delivered message with 'state' sets the recipient's neighbour entry, only delivered target_states refresh its memory / time2forget
//   Greedy targets, and the Heuristic targets that build on them (greedy.py:331-365)   a broadcasting target clears need_communication regardless; recipient t
//                 intersects its non_empty_warehouses with the sets (as held when sent) of the broadcasting senders s whose s -> t copy arrived.  The copy a
//                 broadcast routes to its own sender is an edge like any other (distance 0) and has no other effect.
//   Naive and Random agents send nothing: a channel of their team is inert.  Under a mixture the Greedy agents run for every environment, but only the
//                 environments whose episode drew Greedy (or, targets, Heuristic) have a team that talks: the others' edge rows are zeros.
// Edges: per team two engine-owned int8 matrices [N][n][n], [sender][recipient], behind each launch -- `sent` (what the agents handed to the channel) and
// `delivered` (what arrived: the reference's *_communication_edges).  Both are written for every team that acts in the launch, with or without a channel of its
// own; an environment the launch skips (finished, waiting for the batched restart) and a team that does not act keep their rows.
//
// Out of scope: ExtraCommunicationDelays (a per-pair queue of stale message CONTENTS; its one shared heap breaks the reference's own same-team assertion when
// both teams talk and compares Message objects on ties; "not used in the evaluation script"), and a channel on a camera team played by HeuristicCameraAgent
// (its fallback when the controller's response is lost is a per-camera assignment solve, heuristic.py:70-78): the host refuses that combination.
//
// Draws: one uniform per (team, sender, recipient) and step, only where the team's rate is > 0 (wave-uniform) and the message was sent: a tape
// ([N][n][n] f64, NaN where the reference drew none) or Philox (seed, global environment index, tick, S_CHAN_DROP, sub = team << 8 | sender << 4 | recipient),
// word .x as a 32-bit uniform like the agents' other Bernoulli draws -- independent of first_env_index and of how the batch is sharded.  With a record
// buffer installed the launch stores the uniform each verdict used, NaN where none was drawn.
//
// Lane mapping: the agents' (policy_kernels.hpp).  The camera verdict of (s, c) is computed on the pair lane that runs send_pair, in every round of pairs
// (Nc Nc > 64: up to four); the delay update has used the unfiltered bits by then, send_bits / the `sent` ballot / the neighbour write / `told` see the
// delivered ones.  The target verdict of (s, t) is computed on recipient lane 32 + t while it walks the `needers` bits (the branch on needers != 0 stays
// uniform).  Each verdict lane writes its pair's two edge bytes into an LDS staging area; behind the agents the wave stores the matrices with 4-byte
// stores where n n is a multiple of four (every even team size), byte stores else.  Record rows: one 8-byte store per pair from the verdict lane.
//
// LDS per environment: the stand-alone agents' slice (PolicyPtrs::lds_bytes: agents' record and staging, static and dynamic record, mask words) plus
// channel_staging_bytes(Nc, Nt) = 2 (Nc Nc + Nt Nt) bytes, each matrix rounded up to 4 -- 160 bytes for MATE-4v8-9, 1 KB at 16 / 16.
#pragma once
#include "policy_kernels.hpp"
#include "scripted_rows.hpp"

namespace mate {

enum ChannelStream : uint32_t { S_CHAN_DROP = 26 };       // behind S_SCR_* = 22..25

// Whether one message arrives.  `u`: the pair's uniform (any value where rate == 0), `dist`: norm2 of the two locations (any value where limit < 0),
// `mask`: the pair's mask byte (1 without a mask).
__host__ __device__ inline bool channel_verdict(bool disabled, double limit, double rate, int mask, double u, double dist) {
    if (disabled || mask == 0) return false;
    if (limit >= 0.0 && !(dist <= limit)) return false;
    if (rate > 0.0 && ((rate <= 0.5) ? (u > 1.0 - rate) : (u <= rate))) return false;      // binomial(1, rate) drew 1: dropped
    return true;
}

struct ChannelMixture {               // the team plays an opponent mixture (scripted_rows.hpp): which environments' agents talk at all
    int32_t on, count;
    int32_t kinds[kScriptedKinds];
    double cum[kScriptedKinds];
    const int32_t *episode, *choice;  // [N] each: scripted_opponent_kernel's, as the previous call left them
    const int32_t *tape_choice;       // [N] the team's row of ScriptedDraws::choice, or NULL
};

struct ChannelTeam {
    int32_t set, disabled;            // a channel is set for the team (0: edges only, everything arrives)
    double limit, rate;               // limit < 0: none
    const uint8_t *mask;              // [N][n][n] or NULL
    const double *tape_u;             // [N][n][n] or NULL (Philox)
    double *record_u;                 // [N][n][n] or NULL
    int8_t *sent, *delivered;         // [N][n][n]
    ChannelMixture mix;
};

struct ChannelArgs {
    ChannelTeam team[2];              // MATE_TEAM_CAMERA, MATE_TEAM_TARGET
    int32_t lds_bytes;                // per wave: PolicyPtrs::lds_bytes + channel_staging_bytes, rounded up to 16
};

__host__ __device__ constexpr int channel_matrix_bytes(int n) { return (n * n + 3) & ~3; }
__host__ __device__ constexpr int channel_staging_bytes(int Nc, int Nt) { return 2 * (channel_matrix_bytes(Nc) + channel_matrix_bytes(Nt)); }

// The episode's candidate of a mixture, as scripted_opponent_kernel draws it (restated, not shared: that unit stays as it is): the kind the
// team holds, or at the team's first acting call of an episode the taped kind / the first candidate with u < cum.
__device__ __forceinline__ int channel_mixture_kind(const Params &p, const ChannelMixture &m, int team, int64_t env, int32_t episode) {
    if (m.episode[env] == episode) return m.choice[env];
    const int taped = m.tape_choice ? m.tape_choice[env] : -1;
    bool member = false;
#pragma unroll
    for (int i = 0; i < kScriptedKinds; ++i) member |= i < m.count && m.kinds[i] == taped;
    if (member) return taped;
    const U4 r = philox(p.seed_lo, p.seed_hi, p.first_env + (uint32_t)env, (uint32_t)episode, S_SCR_CHOICE, (uint32_t)team);
    const double u = u53(r.x, r.y);
    int kind = -1;
#pragma unroll
    for (int i = kScriptedKinds - 1; i >= 0; --i)
        if (i < m.count && (u < m.cum[i] || i == m.count - 1)) kind = m.kinds[i];
    return kind;
}

// The Channel policy of greedy_policy_body (see NoChannel there) of one environment.  `stage`: the environment's LDS staging area, zeroed:
// [cameras sent | cameras delivered | targets sent | targets delivered].
struct LiveChannel {
    const Params &p;
    const ChannelArgs &ca;
    const double *st, *dy;
    int8_t *stage;
    int64_t env;
    uint32_t env_global, tick;
    bool talk_c, talk_t;              // the team's agents are the ones whose joint action the step takes (always, but under a mixture)

    __device__ __forceinline__ double uniform(const ChannelTeam &T, int team, int n, int s, int r) const {
        if (T.tape_u) return T.tape_u[(env * n + s) * n + r];
        const U4 w = philox(p.seed_lo, p.seed_hi, env_global, tick, S_CHAN_DROP, (uint32_t)(team << 8 | s << 4 | r));
        return (double)w.x * 2.3283064365386963e-10;
    }
    __device__ __forceinline__ bool verdict(const ChannelTeam &T, int team, int n, int s, int r, double dx, double dy_, double *u_out) const {
        double u = 0.0, dist = 0.0;
        int mask = 1;
        if (T.rate > 0.0) { u = uniform(T, team, n, s, r); *u_out = u; }
        if (T.limit >= 0.0) dist = norm2(dx, dy_);
        if (T.mask) mask = T.mask[(env * n + s) * n + r];
        return channel_verdict(T.disabled != 0, T.limit, T.rate, mask, u, dist);
    }
    __device__ __forceinline__ int camera(int k, int s, int c, int bits) const {
        const ChannelTeam &T = ca.team[0];
        const int Nc = p.Nc;
        double u = __builtin_nan("");
        bool keep = true;
        if (bits != 0 && talk_c) {
            if (T.set) keep = verdict(T, 0, Nc, s, c, st[c] - st[s], st[Nc + c] - st[Nc + s], &u);
            stage[k] = 1;
            stage[channel_matrix_bytes(Nc) + k] = keep ? 1 : 0;
        }
        if (T.record_u) T.record_u[env * (Nc * Nc) + k] = u;
        return keep ? bits : 0;
    }
    __device__ __forceinline__ bool target(int s, int t) const {
        const ChannelTeam &T = ca.team[1];
        const int Nc = p.Nc, Nt = p.Nt;
        double u = __builtin_nan("");
        bool keep = true;
        if (talk_t) {
            const double *x = dy + 2 * Nc, *y = x + Nt;
            if (T.set) keep = verdict(T, 1, Nt, s, t, x[t] - x[s], y[t] - y[s], &u);
            int8_t *m = stage + 2 * channel_matrix_bytes(Nc);
            m[s * Nt + t] = 1;
            m[channel_matrix_bytes(Nt) + s * Nt + t] = keep ? 1 : 0;
        }
        if (T.record_u) T.record_u[(env * Nt + s) * Nt + t] = u;
        return keep;
    }
    __device__ __forceinline__ void targets_done(uint32_t needers, int t) const {      // the record of the pairs nobody sent on
        const ChannelTeam &T = ca.team[1];
        if (!T.record_u) return;
        const int Nt = p.Nt;
        for (int s = 0; s < Nt; ++s)
            if (!((needers >> s) & 1u)) T.record_u[(env * Nt + s) * Nt + t] = __builtin_nan("");
    }
};

// greedy_channel_kernel<float / double observations> on `blocks` workgroups of four environments with `lds` bytes (4 ChannelArgs::lds_bytes); returns the launch's error
hipError_t launch_greedy_channel(bool obs_f64, unsigned blocks, size_t lds, hipStream_t stream, const Params *params, const Ptrs &g, const PolicyPtrs &q, const ChannelArgs &a);
const void *greedy_channel_function(bool obs_f64);      // (for hipFuncSetAttribute)

}  // namespace mate
