// engine_host.h -- the host's state of one engine (struct mate_engine, the environment switches, one struct per attached feature) and the launch plans: the pure
// decisions over that state of which kernel a stepping entry point runs, on how many workgroups, with how much LDS (LaunchPlan), of who plays each team of a call with
// the on-device agents, which launches that takes and whose rows the step consumes (OpponentPlan), and of what is enqueued around the stepping launch in which order
// (AttachedPlan: the ONE place that order is written).  Host only: included by mate_engine.hip, never by the shape-group units; nothing here calls HIP.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mate_engine.h"
#include "reset_kernels.hpp"
#include "reward_rows.hpp"
#include "fragment_rows.hpp"
#include "frame_rows.hpp"
#include "selection_rows.hpp"
#include "opponent_rows.hpp"
#include "state_rows.hpp"
#include "shape_groups.hpp"
#include "headline_kernels.hpp"
#include "episode_rows.hpp"
#include "info_rows.hpp"
#include "scripted_rows.hpp"
#include "channel_rows.hpp"
#include "seat_rows.hpp"
#include "message_rows.hpp"
#include "render_rows.hpp"
#include "trace_rows.hpp"

using namespace mate;

constexpr size_t kLdsCeiling = 160 * 1024;     // LDS one workgroup can have: what a launch's static + dynamic bytes must fit

// Environment switches (all read ONCE, in mate_engine_create; documented in include/mate_engine.h).
struct Switches {
    bool generic = false;          // MATE_GENERIC=1: generic (AnyShape) kernels even for a shape with a compiled specialisation
    bool flow_generic = false;     // MATE_FLOW_GENERIC=1: every launch runs the FLOW_ANY kernel
    int stagger = -1;              // MATE_STAGGER=<5 digits>: per-phase wave priorities of step_kernel (-1: by batch size)
    int lut_small_cap = 0;         // MATE_LUT_SMALL_CAP=<rays>: sort-array size of the small-LDS table launch (0: half the full size)
    bool reset_monolithic = false; // MATE_RESET_MONOLITHIC=1: resets as one launch instead of placement / tables / view
    int rollout_rotate = 1;        // MATE_ROLLOUT_ROTATE=0: no wave-priority rotation in the fused rollouts
    bool no_image = false;         // MATE_NO_IMAGE=1: the fused rollouts pack observations through the descriptor table even where the row-image compilation exists
    bool policy_split = false;     // MATE_POLICY_SPLIT=1: step_greedy / step_versus_greedy as two launches (agents' kernel, step kernel) even when the fused one-launch form applies
    int step_split = -1;           // MATE_STEP_SPLIT=0 / 1: the one-wave / two-wave form of the per-step kernel in the folded flows (-1: by batch size)
    bool zoom_iterate = false;     // MATE_ZOOM_ITERATE=1: the greedy camera agents iterate the zoom solve (greedy.py:139-145) instead of reading its table
    bool step_sub_wave = true;     // MATE_STEP_SUBWAVE=0: the per-step Greedy flows of the small scenarios stay on step_greedy_kernel where the fused ones run sub-wave groups
    int sub_wave_mode = 2;         // MATE_SUBWAVE=0 / 1: one environment per wave in the fused rollouts of the small scenarios too / the shape's number in EVERY fused launch (default 2: where it measured faster, sub_wave_of_launch).  The one switch that changes after create: mate_engine_set_sub_wave
    bool step_greedy_rollout = false;   // MATE_STEP_GREEDY_ROLLOUT=1: the one-launch form of step_greedy / step_versus_greedy on rollout_greedy_kernel with one step (round 3) instead of step_greedy_kernel
    bool pipelined_low_priority = true; // MATE_PIPELINED_PRIORITY=0: the side stream of the pipelined restarts at the default priority instead of the device's lowest
    bool pipelined_serial = false;      // MATE_PIPELINED_SERIAL=1: the pipelined-restart protocol with the resets on the CALLER's stream (the tests' reference)
    bool headline_unit = true;          // MATE_HEADLINE_UNIT=0: the row-image random-policy rollout of MATE-4v8-9 stays on rollout_kernel instead of headline_rollout_kernel (same bytes; the tests' reference, the A/B lever)
};
// ---- attached state, one struct per feature: the launch's arguments, the engine-owned buffers (kept across re-attachments), whether it is on
struct StateRows {       // mate_engine_enable_state_rows: the caller's [N][S] buffer, its type, its (scale, bias) table on the device (null: raw rows)
    void *dst = nullptr; bool f64 = false; const void *ab = nullptr; void *d_ab = nullptr, *d_ab_demand = nullptr;
    std::vector<double> demand_table;            // of the last on-demand call (mate_engine_state_rows): scale[S] | bias[S] | type, as uploaded to d_ab_demand
    bool on() const { return dst != nullptr; }
};
struct RewardRows {      // mate_engine_enable_reward_rows: scalars, masks and mode of `args` are the launch's own
    bool on = false, f64 = false, soft = false, accumulate = false;      // attached; the row type; the soft-coverage launch goes in front; rows += shaped
    RewardArgs args{};
    int32_t *d_snapshot = nullptr; double *d_matrix = nullptr, *d_scores = nullptr;
};
struct Selection {       // mate_engine_enable_selection: phase, masks and scalars of `args` are the launch's own
    bool on = false, act_f64 = true;             // attached; the type of the engine-owned action buffer d_actions, [N][Nc][2]
    SelectionArgs args{};
    double *d_actions = nullptr;
    bool masks_stale = false;                    // a state-only restart (rollout_random's) or import_state ran since the view masks were last written
};
enum RowSource { ROWS_CALLER, ROWS_GREEDY, ROWS_HEURISTIC, ROWS_FINAL };      // whose rows a stepping launch consumes for a team (rows_of): the caller's own, the Greedy agents', the Heuristic launch's, the mixture's final ones
struct Opponents {       // mate_engine_set_camera_opponent / _set_target_opponent, one record per team: the plain selection, what the last call consumed
    int kind[2] = {MATE_OPPONENT_GREEDY, MATE_OPPONENT_GREEDY};      // which scripted agent plays the team where the engine plays it (under a mixture: Heuristic exactly where a candidate needs its machinery)
    int consumed[2] = {ROWS_GREEDY, ROWS_GREEDY};      // the source the last call's stepping launch read for the team (step_with_policies sets it from the plan, the fused launches clear it; mate_engine_policy_actions)
    double *d_drift = nullptr;                   // [N][Nt][2] f64, engine-owned, allocated at the first switch to Heuristic targets: the drift launch's output, the stepping launch's target actions
};
struct CameraOpponent {  // the Heuristic camera agents' tables and memory (opponent_rows.hpp: heuristic_camera_kernel)
    double *d_mesh = nullptr, *d_grid = nullptr, *d_scores = nullptr;      // mate_engine_heuristic_camera_tables: the three tables on the device
    double *d_action = nullptr, *d_prev = nullptr, *d_goals = nullptr;     // [N][Nc][2] f64 each, engine-owned, allocated at the first switch to Heuristic
    int32_t *d_index = nullptr, *d_episode = nullptr;                      // [N][Nc] goal state indices; [N] the episode whose first call has reset the agents
    const int8_t *permutations = nullptr;                                  // mate_engine_heuristic_camera_tape: both hold until replaced
    int8_t *record = nullptr;
    bool ran = false;                            // some call has run the launch since the switch to Heuristic: the Greedy camera agents' memory is behind (switching back marks them for reset)
};
struct ScriptedMixture { // mate_engine_set_opponent_mixture, one per team: the candidates with positive weight, the engine-owned memory of scripted_opponent_kernel (scripted_rows.hpp)
    bool installed = false;                      // the team's setter is refused meanwhile (a single Greedy or Heuristic candidate is that plain selection and nothing else)
    bool launch = false;                         // the team's rows come from the scripted launch: every mixture but {Greedy} and {Heuristic}
    int count = 0, kinds[kScriptedKinds] = {}, frame_skip = 20, restore = MATE_OPPONENT_GREEDY;      // (restore: the plain selection the mixture replaced, back at the clear)
    double cum[kScriptedKinds] = {};
    bool has[kScriptedKinds] = {};
    double *d_final = nullptr, *d_external = nullptr, *d_prev_action = nullptr, *d_prev_location = nullptr, *d_prev_noise = nullptr;      // [N][n][2] each, allocated at the first install that launches
    int32_t *d_episode = nullptr, *d_choice = nullptr, *d_counter = nullptr, *d_goal = nullptr, *d_inc = nullptr;                       // [N], [N], [N], [N][Nt], [N][Nt]
    bool only_greedy() const { return !installed || (count == 1 && kinds[0] == MATE_SCRIPTED_GREEDY); }
};
struct Scripted {        // both teams' mixtures and the draws of their one launch (mate_engine_scripted_tape: both hold until replaced)
    ScriptedMixture team[2];
    ScriptedDraws tape{}, record{};
};
struct Channels {        // mate_engine_set_channel, one per team: the settings, the draws of greedy_channel_kernel (mate_engine_channel_tape: hold until replaced), the engine-owned edge matrices
    struct Team {
        bool set = false, disabled = false;
        double limit = -1.0, rate = 0.0;             // limit < 0: none
        const uint8_t *mask = nullptr;
        const double *tape_u = nullptr; double *record_u = nullptr;
        int8_t *d_sent = nullptr, *d_delivered = nullptr;      // [N][n][n] each, allocated at the first set_channel / channel_edges
    } team[2];
    int lds_bytes = 0;                               // per wave of greedy_channel_kernel (ChannelArgs::lds_bytes), its dynamic LDS opted in: set with the edge matrices
};
struct Seat {            // mate_engine_enable_seat: the learner's seat among the on-device teammates of ONE team (seat_rows.hpp); `spec`, the caller's three buffers, the engine-owned flags
    bool on = false;
    SeatSpec spec{};                             // team, mode, the constant, the team's agents, the caller's tape
    void *obs = nullptr;                         // [N][D_team] obs_dtype: seat_rows_kernel's rows
    int32_t *index = nullptr, *acted = nullptr;  // [N] each: the seat of the row's episode; the seat whose action the last agents' launch consumed
    int32_t *d_live = nullptr;                   // [N], allocated at the first enable: the environments greedy_seat_kernel ran in the call (an idle one keeps its row)
};
struct Messages {        // mate_engine_enable_messages, one per team: the learner's own messages through the team's channel (message_rows.hpp); the caller's three buffers, the draws (mate_engine_message_tape: hold until replaced), the engine-owned edge matrices, counts and tags
    struct Team {
        bool on = false, pairwise = false;
        int width = 0;
        const void *payload = nullptr; const uint8_t *address = nullptr; void *inbox = nullptr;
        const double *tape_u = nullptr; double *record_u = nullptr;
        int8_t *d_sent = nullptr, *d_delivered = nullptr;                          // [N][n][n] each, allocated at the first enable
        int32_t *d_step = nullptr, *d_total = nullptr, *d_agent = nullptr, *d_tags = nullptr;      // [N][n][n], [N][n][n], [N][n][2], [N][2]
    } team[2];
};
struct FragmentRows {    // mate_engine_enable_fragment_rows: scalars, masks, rows and K of `args` are the launch's own; the tables are engine-owned, one set per form
    bool on = false, f64 = false, need_masks = false;     // attached; the shaped rows' type; a mask term had a non-zero coefficient at enable
    FragmentArgs args{};
    double *d_coef = nullptr, *d_coef_demand = nullptr;    // [10] each
    void *d_columns = nullptr, *d_columns_demand = nullptr;      // [max(Dc, Dt)] FragmentColumn<double>-sized entries each
};
struct FirstRows {       // mate_engine_enable_first_rows: the caller's buffers; lives and dies with the fragment rows it completes (team, A, D, obs and column table are theirs)
    bool on = false;
    void *rows = nullptr;                        // [N][A][D] obs_dtype: the restart launch packs the restarted environments' PLAIN first rows here
    float *scalars = nullptr;                    // [N][8]: 2.0f everywhere behind the fragment launch, then the restart's own record (column 2 = 0) where it restarted
    void *final_obs = nullptr;                   // [N][A][D] obs_dtype or null: what the fragment's obs held before the first row replaced it
};
struct FrameFragments {  // mate_engine_enable_frame_fragments: the per-frame fragment (frame_rows.hpp); scalars, rows, reward_rows, phase and closes of `args` are the launch's own
    bool on = false, first_rows = false;
    int team = 0;
    FrameArgs args{};                            // the caller's buffers, K, A, D, the shaped rows' type
    // of the call in progress: set by mate_engine_step_versus_greedy for `team`, cleared when it returns (plan_attached reads them)
    bool in_call = false;                        // the call enqueues the frame launch
    bool closing = false;                        // ... and has enqueued it as the interval's last: its restart carries the second form
    const float *call_scalars = nullptr; const void *call_rows = nullptr;      // ... over these buffers of the call
};
struct EpisodeRecords {  // mate_engine_enable_episode_records: scalars, masks, rows and K of `args` are the launch's own
    bool on = false;
    EpisodeArgs args{};                          // team, A, the caller's ring and counter, the engine-owned sums
    double *d_sums = nullptr;                    // [N][kEpisodeWords], allocated at the first enable: the learner steps of the episodes in progress
};
struct InfoRows {        // mate_engine_enable_info_rows: scalars, masks, mode and done_nan of `args` are the launch's own
    bool on = false;
    InfoArgs args{};                             // the caller's three row buffers (any may be null), the engine-owned snapshot
    int32_t *d_snapshot = nullptr;               // [N][Nt + 1], allocated at the first enable: the goals and the episode the next step's individual_done compares with
};
struct CommTrace {      // mate_engine_enable_comm_trace: RenderCommunication's state (trace_rows.hpp), one matrix per team; the buffers are engine-owned and kept across re-attachments
    int duration = 0;                            // 0: detached
    struct Team {
        bool on = false;
        uint8_t *d_remaining = nullptr;          // [N][n][n], allocated at the first enable
        int32_t *d_tags = nullptr;               // [N]: the episode number the matrix belongs to (-1: none)
        bool call_delivered = false;             // of the call in progress: its agents' launch ran under a channel and wrote the team's `delivered` matrix (step_with_policies sets it, step_launches clears it)
    } team[2];
    bool on() const { return duration > 0; }
};
struct mate_engine {
    Switches sw{};
    hipStream_t last_stream = nullptr;   // stream of the most recent launch: what the host-side accessors wait for ...
    bool launched = false, multi_stream = false;   // ... unless launches went to more than one stream since the last wait (then: the device)
    Params p{};
    Params *d_params = nullptr;   // device copy read by the kernels
    Ptrs g{};
    ResetLds rl{};
    ResetLds rl_small{};       // two-tier table launches (launch_reset): the layout with half-size sort arrays; sort_cap 0 = off
    mate_config cfg{};
    int device = 0;
    int64_t N = 0;
    int parity = 0;
    uint32_t tick = 0;         // Philox tick of the next step launch
    int64_t steps_since_reset = 0;   // batched auto-reset bookkeeping
    bool was_reset = false;
    bool dev_tick = false;     // mate_engine_device_tick: the step counter lives on the device (graph-replayable launches)
    int dev_frames = 1;        // ... frames per launch of the reset interval in progress (1: the per-step flows; K: FrameSkip launches, rollout_versus_greedy)
    int dev_interval = 1;      // ... and the auto-reset interval every step() must then use
    int pending_interval = 0;  // auto_reset value of the batched-reset interval in progress (steps_since_reset > 0)
    // pipelined restarts (mate_engine_rollout_greedy with auto_reset = MATE_RESET_PIPELINED): the side stream the resets run on, the
    // event behind the last rollout launch, one event per list parity behind the reset that consumed that list
    bool pipelined = false;          // records may carry "restarted" tags (Ptrs::pipelined): leave_pipelined() before anything else runs
    int pipe_every = 1, pipe_count = 0;   // ... one restart launch behind every pipe_every-th rollout launch (auto_reset = -pipe_every); launches into the interval
    hipStream_t side = nullptr;
    hipEvent_t ev_launch = nullptr, ev_reset[2] = {nullptr, nullptr};
    bool reset_in_flight[2] = {false, false};
    size_t step_lds = 0, reset_lds = 0;
    KernelSet k{};                 // kernels chosen at create (pick_kernels): shape-specialised when compiled for these counts
    size_t image_wave_bytes = 0;   // per-environment LDS slice of the row-image rollout (k.image), else of the plain one
    int64_t cus = 256;             // compute units of the device
    int split_on = 0;              // launch_step uses k.split (MATE_STEP_SPLIT, or the batch is one resident generation)
    int last_flow = 0;
    std::vector<void *> allocs;
    // on-device rule-based policies (mate_engine_step_greedy)
    bool policy_ready = false;
    PolicyPtrs q{};
    int greedy_team_bits = 0;  // during mate_engine_step_greedy / _step_versus_greedy: teams whose joint action the policy kernel wrote
    // observation post-processing fused into the packer (set_obs_mode / set_obs_transform)
    int team_mode[2] = {0, 0};      // per team (set_obs_mode)
    bool xf_relative = false, xf_cam = false, xf_tgt = false;
    std::vector<double> xf_cam_scale, xf_cam_bias, xf_tgt_scale, xf_tgt_bias;
    uint2 *d_xdesc = nullptr;
    void *d_xab = nullptr;
    Opponents opponents;       // who plays each team where the engine plays it, whose rows the last call consumed -- what a CALL makes of these four: plan_opponents
    CameraOpponent camera_opponent;      // the Heuristic camera agents' tables and memory
    Scripted scripted;                   // the opponent mixtures
    Channels channel;                    // the communication channels
    Seat seat;                           // the learner's seat among on-device teammates
    Messages messages;                   // the learner's own messages through the team's channel
    CommTrace trace;                     // RenderCommunication's per-pair countdowns
    StateRows state; RewardRows reward; Selection selection; FragmentRows fragment; FirstRows first; FrameFragments frames; EpisodeRecords episodes; InfoRows info;      // what is attached around the stepping launches (plan_attached)
    // kernel timing (HIP events on the launch stream)
    int timing = 0;            // 0 = off, k = time every k-th step launch
    int64_t timing_tick = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t events_used = 0;
};

// ---- launch plans
// What a stepping entry point launches is decided HERE, as a value, by pure functions of the engine (and of the call's record pointers where
// the flow depends on them): no HIP call, no allocation, nothing written, no environment variable read.  Everything else reads the plan: the launch sites launch
// it and compute no geometry, policy_enable opts in what plan_with_policies can return, step_with_policies asks whether it fits, set_sub_wave reports its E.
struct LaunchPlan {
    StepFn step = nullptr; PolicyFn policy = nullptr;      // the kernel: of launch_step and rollout_random_impl, or of rollout_with_policies
    int E = 1;                                             // environments per wave (engine_kernels.hpp, Ctx<ObsT, L>)
    unsigned blocks = 0, threads = 256;
    size_t lds = 0;                                        // dynamic LDS per workgroup
    int last_flow = FLOW_ANY;                              // what mate_engine_last_flow reports behind the launch
    bool fits() const { return lds <= kLdsCeiling; }
};
static unsigned blocks_of(const mate_engine *e, int envs_per_block) { return (unsigned)((e->N + envs_per_block - 1) / envs_per_block); }

// Environments per wave the sub-wave kernels of a flow run with: the shape's E = 4 (2: MATE-4v8-0's Greedy flows) where they exist and
//   mode 1: always;
//   mode 2: where they measured faster (profiles/r06_subwave_probe.txt) -- batches of at least 32 environments per CU (8192 on an MI355X:
//           below that a launch has one wave per SIMD or less and is latency-bound whatever the lane use: x0.6 .. 1.1 at 4096), and,
//           under the random policy, every shape but MATE-4v4-*, whose one-per-wave rollout (the register-resident row image) is as fast.
//           Greedy flows x1.2 .. 3.3, random-policy flows x1.1 .. 2.9 there.
static int sub_wave_of_launch(const mate_engine *e, bool greedy) {
    const int mode = e->sw.sub_wave_mode;
    if (mode == 0 || e->k.sub_wave <= 1 || !(greedy ? (const void *)e->k.rollout_greedy_sub : (const void *)e->k.rollout_sub[0])) return 1;
    if (mode == 1) return e->k.sub_wave;
    if (e->N < 32 * e->cus) return 1;
    if (!greedy && e->p.Nc * e->p.Nt >= 16) return 1;      // MATE-4v4-*: the row-image kernel is as fast or faster (x0.72 .. 1.14)
    return e->k.sub_wave;
}
// The compilation for the call's switches (enum Flow), when they are the common ones
static int folded_flow(const mate_engine *e, int mode, const Ptrs &g) {
    const bool common = !e->sw.flow_generic && !g.tape_ct && !g.tape_goal && !g.act_discrete && g.obs_mode == 0 && !g.xdesc && !g.xab &&
                        g.scratch_init && (g.cam_obs || e->p.Nc == 0) && g.tgt_obs && g.scalars;
    if (common && mode == MODE_STEP_RANDOM) return FLOW_RANDOM;
    if (common && mode == MODE_STEP) return FLOW_ACT_F32;      // caller-supplied real-valued actions, f32 or f64 per team
    return FLOW_ANY;
}

// step() / step_random() / observe(); `g`: the call's record pointers (apply_io), mode set
static LaunchPlan plan_step(const mate_engine *e, int mode, const Ptrs &g) {
    LaunchPlan pl;
    const int flow = pl.last_flow = folded_flow(e, mode, g);
    // The small scenarios' steps on the sub-wave rollout kernel with ONE step (Ptrs::per_step; the same switches folded as in step_kernel), where
    // their fused flows run it: from 32 environments per CU on.  Every mode but observe(); MATE_STEP_SUBWAVE=0 keeps the per-step kernels.
    pl.E = (mode != MODE_OBSERVE && e->sw.step_sub_wave && !e->p.obs_f64) ? sub_wave_of_launch(e, false) : 1;
    if (pl.E > 1) { pl.step = e->k.rollout_sub[flow]; pl.blocks = blocks_of(e, 4 * pl.E); pl.lds = pl.E * e->step_lds; }
    else if (e->split_on && e->k.split[flow]) { pl.step = e->k.split[flow]; pl.blocks = blocks_of(e, 1); pl.threads = 128; pl.lds = e->step_lds / 4; }      // two waves per environment: one 128-thread workgroup each
    else { pl.step = e->k.step[flow]; pl.blocks = blocks_of(e, 4); pl.lds = e->step_lds; }
    return pl;
}
// The engine's row-image random-policy rollout is the headline's form -- the compiled MATE-4v8-9 set with its row image, f32 rows -- and the library has
// headline_rollout_kernel (headline_kernels.hpp; a profiling build has none): which launches run it is plan_rollout_random's choice.
static bool headline_form(const mate_engine *e) {
    return e->k.specialised && e->k.image && !e->p.obs_f64 && e->p.Nc == 4 && e->p.Nt == 8 && e->p.No == 9 && headline_rollout_function(0) != nullptr;
}
// rollout_random(); `g`: the call's record pointers, tapes cleared
static LaunchPlan plan_rollout_random(const mate_engine *e, const Ptrs &g) {
    LaunchPlan pl;
    const int flow = pl.last_flow = folded_flow(e, MODE_STEP_RANDOM, g);
    pl.E = sub_wave_of_launch(e, false);
    pl.blocks = blocks_of(e, 4 * pl.E);
    if (pl.E > 1) { pl.step = e->k.rollout_sub[flow]; pl.lds = pl.E * e->step_lds; }
    else { pl.step = e->k.rollout[flow]; pl.lds = (flow == FLOW_RANDOM && e->k.image) ? 4 * e->image_wave_bytes : e->step_lds; }
    // the headline's own kernel in place of rollout[FLOW_RANDOM], the instantiation of the launch's store form: same rows, same flow reported
    // (MATE_HEADLINE_UNIT=0: never; a launch with a debug hook set -- phase clocks, a skip mask -- keeps the kernel that honours it)
    if (pl.E == 1 && flow == FLOW_RANDOM && e->sw.headline_unit && headline_form(e) && !g.phase_clocks && !g.debug_skip) {
        pl.step = headline_rollout_function(g.store_shifted);
        pl.lds = headline_lds_bytes(e->image_wave_bytes);
    }
    return pl;
}
// The three kernels a launch with the on-device agents can be, each with its workgroup's LDS: the environments' slices and the agents' (+ 1024 bytes: the
// exchange area of the zoom solve the agents once shared -- nothing reads it since the solve became a table lookup; the one-per-wave rollout keeps its size, the sub-wave
// launches, whose occupancy the LDS bounds, do without).  The caller plays the cameras: step_greedy_kernel holds the target agents' section only (one more workgroup per CU).
enum PolicyForm { FORM_ROLLOUT, FORM_ROLLOUT_SUB, FORM_STEP_GREEDY, kPolicyForms };
static LaunchPlan policy_form(const mate_engine *e, int form, int team_caller) {
    const Params &p = e->p;
    LaunchPlan pl;
    pl.policy = form == FORM_STEP_GREEDY ? e->k.step_greedy : form == FORM_ROLLOUT_SUB ? e->k.rollout_greedy_sub : e->k.rollout_greedy;
    pl.last_flow = form == FORM_STEP_GREEDY ? FLOW_STEP_GREEDY : FLOW_GREEDY;
    pl.E = form == FORM_ROLLOUT_SUB ? e->k.sub_wave : 1;
    pl.blocks = blocks_of(e, 4 * pl.E);
    const int slice = form == FORM_STEP_GREEDY ? step_greedy_slice_bytes(e->q.PW, e->q.TW, p.Nc, p.Nt, p.MW, team_caller != 0) : policy_slice_bytes(e->q.PW, p.Nc, p.Nt);
    pl.lds = (size_t)pl.E * (4 * (size_t)p.lds_wave_bytes + 4 * (size_t)slice) + (form != FORM_STEP_GREEDY && pl.E == 1 ? 1024 : 0);
    return pl;
}
// rollout_greedy() / rollout_versus_greedy() and (`per_step`) the one-launch step_greedy() / step_versus_greedy().  The fused rollouts run rollout_greedy_kernel, E
// environments per wave where the sub-wave workgroup fits; the per-step flows follow them there (its one-step form: MATE-2v4-0 x 16 384 against the greedy cameras
// 38.2 -> 20.5 us per step, x1.2 .. 1.9 from 8192 environments on; same bytes; MATE_STEP_SUBWAVE=0: not) and run step_greedy_kernel (step_kernel's sequence with
// the agents in front) elsewhere, where it exists and fits -- MATE_STEP_GREEDY_ROLLOUT=1: rollout_greedy_kernel with one step.
static LaunchPlan plan_with_policies(const mate_engine *e, bool per_step, int team_caller) {
    const bool sub = (!per_step || e->sw.step_sub_wave) && sub_wave_of_launch(e, true) > 1 && policy_form(e, FORM_ROLLOUT_SUB, team_caller).fits();
    const bool light = per_step && !sub && e->k.step_greedy && !e->sw.step_greedy_rollout && policy_form(e, FORM_STEP_GREEDY, -1).fits();
    return policy_form(e, sub ? FORM_ROLLOUT_SUB : light ? FORM_STEP_GREEDY : FORM_ROLLOUT, team_caller);
}

// ---- the attached launches
// What a call enqueues AROUND its stepping (or reset / import) launch, in the order of the fields: THE one place that order is written.  The "attached
// launches" section of mate_engine.hip has one function per position; each reads this plan and launches what it names, with the geometry it carries.
//   1 execute      selection_kernel, SELECTION_EXECUTE: the camera team's joint action of this frame       attached_ahead_of_step (step_selected)
//   2              the stepping launch (and, two-launch form, the opponents' agents in front of it)
//   2a..2c         the two-launch form's launches between the two, in this order: the agents' launch (policy_kernel or greedy_channel_kernel),     step_with_policies
//                  heuristic_camera_kernel, heuristic_drift_kernel, scripted_opponent_kernel -- WHICH of them a call runs, for which teams, and whose
//                  rows the stepping launch then consumes is the call's OpponentPlan (plan_opponents, below)
//   2d trace       comm_trace_kernel, behind the agents' launches (their `delivered` edges, the learner's routed step_edges) and ahead of the stepping     step_launches, rollout_with_policies
//                  launch, as the wrapper updates before env.step: the per-pair countdowns of RenderCommunication (trace_rows.hpp)
//   3 reward       soft_coverage_kernel where the term exists, reward_rows_kernel: the step's rows          attached_behind_step
//   3b info        info_rows_kernel: MoreTrainingInformation's per-agent rows of the launch's last frame       attached_behind_step
//   4 observe      selection_kernel, SELECTION_OBSERVE: the selection metrics against that step's masks     attached_behind_step
//   5 fragment     fragment_rows_kernel over the K frames of a fused learner-versus-greedy launch           attached_behind_step
//   5' frame       fragment_frame_kernel behind a mate_engine_step_versus_greedy call of the attached team: that frame into the     attached_behind_step
//                  per-frame fragment (frame_rows.hpp) -- the fused fragment's position
//   5b first_rows  a memset node: every record of the first-row scalars reads 2.0f, "not restarted"          attached_behind_step
//   5c episodes    episode_rows_kernel over the call's frames: the learner steps into the episodes' running    attached_behind_step
//                  sums, one record per episode that ends (it reads 3's rows)
//   6              the restart epilogue, a reset or an import (first_rows: the fused call's own restart      restart_finished
//                  stores the learner team's plain first rows and its record into the first-row buffers)
//   6b first_rows  behind THAT restart only: fragment_rows_kernel, K = 1, twice over the restart's records   attached_behind_restart
//                  -- obs -> final_obs (plain copy; where asked for), then first rows -> obs (column table)
//   6b' frame      behind the restart of the call that closes an interval, where first rows were asked for: fragment_frame_kernel's     attached_behind_restart
//                  second form -- obs -> final_obs, the call's rows (now the first rows) -> obs, restarted = 1
//   6c             with reward rows the snapshot-only launch; with info rows theirs                        attached_behind_restart
//   7 action_mask  selection_kernel, SELECTION_ACTION_MASK: of the rows the learner sees next               attached_last
//   8 state        state_rows_kernel, last                                                                  attached_last
//   9 seat         seat_rows_kernel behind everything of a mate_engine_step_seated call: the seat's row, the seat      seat_rows_behind
struct Tiles { unsigned blocks = 0, threads = 256; size_t lds = 0; int E = 0; };      // grid, workgroup, dynamic LDS, environments per workgroup (blocks 0: no launch)
struct AttachedPlan {
    bool execute = false, reward = false, observe = false, fragment = false, first_rows = false, frame = false, frame_first = false, episodes = false, info = false, action_mask = false, state = false;
    Tiles soft_coverage, reward_rows, selection, fragment_rows, frame_rows, episode_rows, info_rows, state_rows;      // (selection: the three phases are one kernel on one grid)
};
static Tiles plan_attached_tile(const mate_engine *e) { return {blocks_of(e, kAttachedEnvsPerBlock), 256, (size_t)attached_tile_lds_bytes(e->p.DW), kAttachedEnvsPerBlock}; }      // the shared tile of attached_tile.hpp
static Tiles plan_soft_coverage(const mate_engine *e) { return {(unsigned)((e->N * e->p.Nc + 3) / 4), 256, 0, 0}; }      // a wave per (environment, camera)
// Environments per workgroup: 16, or fewer where the tile (records + rows of the type) would take more than 40 KB of LDS
static Tiles plan_state_rows(const mate_engine *e, bool f64) {
    const Params &p = e->p;
    const int S = state_dim_of(p.Nc, p.Nt, p.No), sz = f64 ? 8 : 4;
    int E = 16;
    while (E > 4 && state_rows_lds_bytes(p.SW, p.DW, S, E, sz) > 40 * 1024) E /= 2;
    return {blocks_of(e, E), 256, (size_t)state_rows_lds_bytes(p.SW, p.DW, S, E, sz), E};
}
static Tiles plan_fragment_rows(const mate_engine *e) { return {blocks_of(e, kAttachedEnvsPerBlock), 256, 0, kAttachedEnvsPerBlock}; }
// A workgroup per tile, or ONE for all of them where the ring is smaller than the batch (episode_rows.hpp: the serial form)
static Tiles plan_episode_rows(const mate_engine *e) { return {e->episodes.args.capacity < e->N ? 1u : blocks_of(e, kAttachedEnvsPerBlock), 256, 0, kAttachedEnvsPerBlock}; }
static Tiles plan_info_rows(const mate_engine *e) {
    return {blocks_of(e, kAttachedEnvsPerBlock), 256, (size_t)info_rows_lds_bytes(e->p.DW, e->p.Nc, e->p.Nt), kAttachedEnvsPerBlock};
}
// `selected`: the call is mate_engine_step_selected; `fused_team`: the call is mate_engine_rollout_versus_greedy for that team (-1: any other).  The action mask is the view the executor would act on next, so while selection is
// attached it follows every call that leaves new records (a reset and observe() too), as long as the engine's mask words are current.
static AttachedPlan plan_attached(const mate_engine *e, bool selected, int fused_team = -1) {
    AttachedPlan pl;
    pl.execute = pl.observe = selected;
    pl.action_mask = e->selection.on && e->selection.args.action_mask && !e->selection.masks_stale;
    pl.reward = e->reward.on;
    pl.fragment = e->fragment.on && fused_team == e->fragment.args.team;
    pl.first_rows = pl.fragment && e->first.on;
    pl.frame = e->frames.on && e->frames.in_call;
    pl.frame_first = pl.frame && e->frames.closing && e->frames.first_rows;
    if (pl.frame) pl.frame_rows = plan_fragment_rows(e);
    pl.episodes = e->episodes.on;
    pl.info = e->info.on;
    pl.state = e->state.on();
    if (e->reward.soft) pl.soft_coverage = plan_soft_coverage(e);
    pl.reward_rows = pl.selection = plan_attached_tile(e);
    pl.fragment_rows = plan_fragment_rows(e);
    if (pl.episodes) pl.episode_rows = plan_episode_rows(e);
    if (pl.info) pl.info_rows = plan_info_rows(e);
    pl.state_rows = plan_state_rows(e, e->state.f64);
    return pl;
}

// ---- the opponents
// Who plays each team of ONE call with the on-device agents (`team_caller`: -1 both teams are the engine's, else the caller's team), which launches that takes
// and whose rows the stepping launch consumes.  Everything else reads this: one_launch_step and step_with_policies (the launches, in the order of the fields),
// rollout_with_policies (the refusal), scripted_team_args, channel_args.
// `seat_team`: the call is mate_engine_step_seated (or the question whether it could be: mate_engine_enable_seat and the setters ask HERE) with the learner's
// seat on that team -- both teams are the engine's, the seat team's Greedy agents act around the seat in greedy_seat_kernel, its rows stay the Greedy buffer.
enum FusedRefusal { FUSED_OK, FUSED_MIXTURE, FUSED_CHANNEL, FUSED_HEURISTIC };
enum SeatRefusal { SEAT_OK, SEAT_HEURISTIC, SEAT_MIXTURE, SEAT_CHANNEL, SEAT_OPPOSING_CHANNEL };      // what of the engine's state a seat on `seat_team` cannot live with
struct OpponentPlan {
    struct Team {
        bool engine = false;       // the engine plays the team in this call: not the caller's, and it has agents (a scenario without cameras: every camera selection is a no-op)
        int source = ROWS_CALLER;  // whose rows the stepping launch consumes (rows_of)
        bool greedy = false;       // its Greedy agents act in the agents' launch: they play, or a candidate of the mixture needs their row (the Heuristic targets build on it)
        bool heuristic = false;    // its Heuristic launch runs: heuristic_camera_kernel in the Greedy cameras' place / heuristic_drift_kernel behind the Greedy targets
        bool scripted = false;     // it is in the scripted launch: a mixture whose rows come from scripted_opponent_kernel
        bool channel = false;      // its channel is live: set, and its communicating agents act -- the Greedy ones, or the Heuristic targets that inherit the Greedy targets' exchange
    } team[2];
    bool agents = false;           // there is an agents' launch ...
    int caller_team = -1;          // ... with this q.caller_team (the team whose Greedy agents sit out; -1: neither) ...
    bool channel_kernel = false;   // ... and it is greedy_channel_kernel (channel_rows.hpp)
    Tiles drift_rows;              // the drift launch's geometry (blocks 0: none)
    bool one_launch = true;        // the opponents allow the one-launch step: plain Greedy agents, no live channel, no seat
    bool seat = false;             // the agents' launch is greedy_seat_kernel (seat_rows.hpp)
    int seat_refusal = SEAT_OK;    // why a seat on `seat_team` is refused: its teammates must be plain Greedy agents without a channel, and the opposing team's channel not live
    int refusal = FUSED_OK, refusal_team = -1;      // why a fused K-frame launch is refused (their kernels hold the Greedy agents and deliver every message), and for which team
};
static int agents_of(const mate_engine *e, int team) { return team == MATE_TEAM_CAMERA ? e->p.Nc : e->p.Nt; }
// THE one mapping of a source to the buffer a stepping launch reads for `team` (null: the caller's own pointer)
static const double *rows_of(const mate_engine *e, int team, int source) {
    switch (source) {
    case ROWS_GREEDY: return team == MATE_TEAM_CAMERA ? e->q.cam_act : e->q.tgt_act;
    case ROWS_HEURISTIC: return team == MATE_TEAM_CAMERA ? e->camera_opponent.d_action : e->opponents.d_drift;
    case ROWS_FINAL: return e->scripted.team[team].d_final;
    default: return nullptr;
    }
}
static OpponentPlan plan_opponents(const mate_engine *e, int team_caller, int seat_team = -1) {
    OpponentPlan pl;
    pl.seat = seat_team >= 0;
    for (int team = 0; team < 2; ++team) {
        OpponentPlan::Team &t = pl.team[team];
        const ScriptedMixture &m = e->scripted.team[team];
        const bool camera = team == MATE_TEAM_CAMERA;
        t.engine = team != team_caller && agents_of(e, team) > 0;
        t.heuristic = t.engine && e->opponents.kind[team] == MATE_OPPONENT_HEURISTIC;
        t.scripted = t.engine && m.launch;
        t.source = team == team_caller ? ROWS_CALLER : t.scripted ? ROWS_FINAL : t.heuristic ? ROWS_HEURISTIC : ROWS_GREEDY;      // (nobody to play: the Greedy buffer, empty)
        t.greedy = team != team_caller && (t.scripted ? m.has[MATE_SCRIPTED_GREEDY] || (!camera && m.has[MATE_SCRIPTED_HEURISTIC]) : camera ? !t.heuristic : true);
        t.channel = e->channel.team[team].set && t.engine && t.greedy && !(camera && t.heuristic);
        // the refusals in the order rollout_with_policies has always checked them: a mixture of either team (camera first), a channel (camera first), the Heuristic targets, the Heuristic cameras
        if (t.engine && !m.only_greedy() && pl.refusal != FUSED_MIXTURE) { pl.refusal = FUSED_MIXTURE; pl.refusal_team = team; }
    }
    const OpponentPlan::Team &c = pl.team[MATE_TEAM_CAMERA], &t = pl.team[MATE_TEAM_TARGET];
    if (pl.refusal == FUSED_OK && (c.channel || t.channel)) { pl.refusal = FUSED_CHANNEL; pl.refusal_team = c.channel ? MATE_TEAM_CAMERA : MATE_TEAM_TARGET; }
    if (pl.refusal == FUSED_OK && (c.heuristic || t.heuristic)) { pl.refusal = FUSED_HEURISTIC; pl.refusal_team = t.heuristic ? MATE_TEAM_TARGET : MATE_TEAM_CAMERA; }
    pl.agents = c.greedy || t.greedy;
    pl.caller_team = c.greedy && t.greedy ? -1 : c.greedy ? MATE_TEAM_TARGET : MATE_TEAM_CAMERA;
    pl.channel_kernel = c.channel || t.channel;
    if (t.heuristic) pl.drift_rows = plan_attached_tile(e);
    pl.one_launch = !c.heuristic && !t.heuristic && !c.scripted && !t.scripted && !pl.channel_kernel && !pl.seat;
    if (pl.seat) {
        const OpponentPlan::Team &other = pl.team[1 - seat_team];
        pl.seat_refusal = e->opponents.kind[seat_team] == MATE_OPPONENT_HEURISTIC ? SEAT_HEURISTIC : !e->scripted.team[seat_team].only_greedy() ? SEAT_MIXTURE
                        : e->channel.team[seat_team].set ? SEAT_CHANNEL : other.channel ? SEAT_OPPOSING_CHANNEL : SEAT_OK;
    }
    return pl;
}
