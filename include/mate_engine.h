/* mate_engine.h -- C ABI of the MI355X-native batched MultiAgentTracking step engine.
 *
 * The upstream reference (XuehaiPan/mate) has no FFI: the boundary its callers use is the
 * Python class mate.environment.MultiAgentTracking (mate/environment.py:288) reached through
 * mate.make (mate/__init__.py:24-46).  This header is the C-ABI a binding for that class
 * sits on; every entry point names the reference method it stands in for.  Plain pointers
 * and sizes only: all `*_dev` pointers are DEVICE pointers (e.g. torch `.data_ptr()`),
 * caller-owned, never freed by the engine.  `stream` is a hipStream_t passed as void*
 * (NULL = the default stream); calls on one handle must be serialised by the caller.
 * Every function returns 0 on success or a negative MATE_E* code; the message is available
 * from mate_engine_last_error().  One handle drives N independent environments on one GPU.
 *
 * Synchronisation.  Launching entry points only enqueue on `stream`.  The host-side accessors without a stream
 * argument (seed, lut_read / lut_write(_outer), set_obs_transform, set_obs_mode, set_action_grids,
 * enable_outer_boundary, idle_steps, kernel_time) wait for the stream of the handle's MOST RECENT launch
 * (hipStreamSynchronize), never for the whole device: other streams of the caller keep running.  Exception: a caller that
 * launched through this handle on MORE than one stream since the last such wait, or that has destroyed that stream, gets
 * hipDeviceSynchronize instead -- an accessor never touches engine memory under a launch in flight.
 *
 * Environment switches.  All are read ONCE, in mate_engine_create(), and fixed for the life of the handle; none
 * changes results (each selects between implementations the tests hold bit-identical, except MATE_ZOOM_ITERATE,
 * see below).  They exist for tests and measurements:
 *   MATE_GENERIC=1           run the generic kernels even for a (cameras, targets, obstacles) shape with a compiled
 *                            specialisation (mate_layout.specialised reports which one runs).  Compiled: the shapes of all
 *                            seventeen scenarios the reference ships (csrc/shape_groups.hpp); a generic fused rollout runs
 *                            at less than half the rate of a specialised one
 *   MATE_FLOW_GENERIC=1      run the kernel that reads every launch switch at run time instead of the ones compiled
 *                            for the common flows (mate_engine_last_flow)
 *   MATE_STAGGER=<digits>    wave priorities of the single-step kernel at its five phase boundaries, one decimal digit
 *                            (0-3) each, e.g. 33210; default 0 = off (round 4: they cost 3 % once the rows leave early)
 *   MATE_ROLLOUT_ROTATE=0    no per-step rotation of the wave priorities in the fused rollout kernels (default 1; 8..20: the
 *                            turn follows the shader clock >> n instead of the wave's step count -- measured, no gain)
 *   MATE_RESET_MONOLITHIC=1  whole-batch / masked / batched resets as ONE launch instead of placement, per-camera
 *                            occlusion tables and first view as separate launches
 *   MATE_LUT_SMALL_CAP=<n>   ray capacity of the small-LDS occlusion-table launch (default: half of the worst case);
 *                            tables with more rays are built by the full-size launch behind it
 *   MATE_NO_IMAGE=1          the fused rollouts pack observations through the descriptor table even for a shape with a
 *                            row-image compilation (same rows; tests compare the two)
 *   MATE_HEADLINE_UNIT=0     the fused random-policy rollout of MATE-4v8-9 (f32 rows, row image, one environment per wave) stays on
 *                            rollout_kernel instead of the kernel compiled for that one form (headline_rollout_kernel; same bytes:
 *                            tests compare the two, benchmarks use it as the A/B lever)
 *   MATE_POLICY_SPLIT=1      mate_engine_step_greedy / _step_versus_greedy as two launches (the agents' kernel, then the step
 *                            kernel) even where the fused one-launch form applies (same results; tests compare the two)
 *   MATE_STEP_GREEDY_ROLLOUT=1  the one-launch form of mate_engine_step_greedy / _step_versus_greedy on the fused rollout kernel with a
 *                            single step (rounds 3-4) instead of step_greedy_kernel (policy_kernels.hpp: the per-step kernel's own
 *                            sequence with the agents in front; same results, tests compare the two)
 *   MATE_STEP_SPLIT=0|1      the per-step kernel of the folded flows (step_random / step with real-valued actions, f32 observations)
 *                            as one wave per environment (0) or two (1: cameras, sector tests and goals on one wave, targets
 *                            and range tests on the other; engine_kernels.hpp: step_split_kernel); default: by what measured
 *                            faster at the batch size (profiles/HISTORY.md 3.1d); the same bytes either way (tests compare the two)
 *   MATE_ZOOM_ITERATE=1      the on-device GreedyCameraAgent runs the reference's 20-iteration zoom solve
 *                            (mate/agents/greedy.py:139-145) instead of reading its tabulation; the two differ by
 *                            <= 1.5e-13 degrees in the viewing angle (parity runs that want the iteration itself)
 *   MATE_BLOCK_FREE_RANGE=1  mate_engine_block_free also gives the block's virtual address range back (hipMemAddressFree) instead
 *                            of keeping it reserved for the life of the process (read once, at the first block_free).  Unsafe on
 *                            this driver: a range handed out again lost stores of the next kernel (tools/va_reuse.hip)
 *   MATE_BLOCK_DEAD_GIB=g    address space [GiB] that freed blocks may keep reserved per process (default 4096 of the 131072 a process
 *                            has): beyond it mate_engine_block_alloc fails with MATE_ENOMEM and the caller uses plain device memory
 *                            (read once, at the first block_alloc)
 *   MATE_PIPELINED_SERIAL=1  pipelined restarts (MATE_RESET_PIPELINED) with the resets on the caller's stream: the reference form
 *                            the tests compare the concurrent one with; MATE_PIPELINED_PRIORITY=0: the side stream at the default
 *                            priority instead of the device's lowest (both read when the mode is first entered)
 *   MATE_SUBWAVE=0|1         environments per wave of the fused rollouts of the small scenarios (mate_engine_set_sub_wave below): 0 = always
 *                            one, 1 = the shape's number (four; two for MATE-4v8-0's Greedy flows) in every such launch; default: where it
 *                            measured faster.  MATE_STEP_SUBWAVE=0: the per-step mate_engine_step / _step_random / _step_greedy /
 *                            _step_versus_greedy keep the per-step kernels where the fused flows run sub-wave groups (default: they follow,
 *                            as one-step launches of the same kernels).  Same bytes either way.
 * Read by the Python host: MATE_ENGINE_LIB=<path> (mate_amd/_native.py: another build of this library, e.g. the profiling build
 * lib/libmate_engine_prof.so); MATE_BUILD_JOBS=<n> (mate_amd/build.py: parallel hipcc processes, default one per translation
 * unit up to the CPU count); and (mate_amd/engine.py), once, when an Engine object is built -- they steer where
 * Engine.reserve_rollout puts the [steps][N][...] observation blocks of the fused rollouts, never what is written there:
 *   MATE_PLAIN_BLOCKS=1      blocks from torch.zeros instead of mate_engine_block_alloc
 *   MATE_BLOCK_CANDIDATES=n  at most n candidates probed per block (default 3, allocated side by side; 6 and -- for the target block --
 *                            as many as the memory and time bounds allow in a deep search; n <= 1: one block, unprobed)
 *   MATE_BLOCK_DEEP=1        the deep search (candidates separated by unmapped 12 GB spacers: a walk through the device's memory)
 *                            for the target block even when reserve_rollout is not asked for it (search='deep': bench.py does;
 *                            off by default since round 5 -- a co-resident learner should not see 45 % of the HBM vanish for seconds)
 *   MATE_BLOCK_SECONDS=s     wall-time bound of the search (default 0.3; deep: 3)
 *   MATE_BLOCK_GIB=g         bound of the deep search's transient footprint in GiB (default 96; always at most 45 % of the free memory)
 *   MATE_STORE_FORM=0|1      force the form of the row stores (mate_engine_set_store_form) instead of choosing by the probed rate
 */
#ifndef MATE_ENGINE_H
#define MATE_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Stays 1: everything added since (mate_engine_enable_state_rows / mate_engine_state_rows, mate_engine_enable_reward_rows, target selection, fragment rows, first rows, the target and camera opponents, the per-frame fragments) is purely additive -- new symbols,
 * no change to a struct or to an existing entry point's arguments -- so a binding built against the older header keeps working. */
#define MATE_ABI_VERSION 1

enum {
    MATE_OK = 0,
    MATE_EINVAL = -1,   /* bad argument / configuration (reference: ValueError / AssertionError) */
    MATE_EHIP = -2,     /* a HIP runtime call failed */
    MATE_ENOMEM = -3,
    MATE_ESTATE = -4    /* call sequence error (e.g. step before reset) */
};

enum { MATE_OBS_F32 = 0, MATE_OBS_F64 = 1 };
enum { MATE_ACT_F32 = 0, MATE_ACT_F64 = 1,
       /* OR-ed into act_dtype: that team's joint action is int32 grid indices [N][agents] instead of [N][agents][2]
        * reals (DiscreteCamera / DiscreteTarget, mate/wrappers/discrete_action_spaces.py:59-74, 165-180);
        * the grids come from mate_engine_set_action_grids */
       MATE_ACT_CAMERA_DISCRETE = 0x100, MATE_ACT_TARGET_DISCRETE = 0x200 };

/* Scenario description = the validated YAML/JSON/dict configuration of the reference
 * (mate/environment.py:113-269: read_config + validate_config), flattened. */
typedef struct mate_config {
    int32_t num_cameras, num_targets, num_obstacles;
    int32_t max_episode_steps;            /* environment.py:199-203 */
    int32_t sparse_reward;                /* reward_type == 'sparse', environment.py:526 */
    int32_t num_cargoes_per_target;       /* environment.py:223-229 */
    int32_t shuffle_entities;             /* environment.py:253-256 */
    int32_t targets_start_with_cargoes;   /* environment.py:240-243 */
    double high_capacity_target_split;    /* environment.py:231-238 */
    double bounty_factor;                 /* environment.py:245-251 */
    double transmittance;                 /* obstacle/transmittance, environment.py:1470-1476 */
    double camera_radius, camera_min_viewing_angle, camera_max_sight_range;
    double camera_rotation_step, camera_zooming_step;   /* entities.py:248-254 */
    double target_step_size, target_sight_range;        /* entities.py:563-566 */
    double obstacle_radius_range[2];      /* radius_random_range (lo, hi) */
    const double *camera_location_ranges;   /* [num_cameras][4]  = x_lo, x_hi, y_lo, y_hi (host memory) */
    const double *target_location_ranges;   /* [num_targets][4] */
    const double *obstacle_location_ranges; /* [num_obstacles][4] */
    int32_t obs_dtype;                    /* MATE_OBS_F32 (default product path) or MATE_OBS_F64 */
} mate_config;

/* Sizes and the bit layout of the packed visibility masks, for the binding. */
typedef struct mate_layout {
    int32_t camera_obs_dim, target_obs_dim, state_dim;   /* constants.py:267-300, environment.py:450-466 */
    int32_t mask_words;          /* u32 words per environment in the packed mask export */
    int32_t bit_camera_target;   /* bit(c,t)  = bit_camera_target + c*Nt + t       (environment.py:1364-1367) */
    int32_t bit_camera_camera;   /* bit(c,c') = bit_camera_camera + c*Nc + c'      (environment.py:1381-1386) */
    int32_t bit_target_row;      /* bit(t,j)  = bit_target_row + t*(Nc+No+Nt) + j, j: cameras, obstacles, targets */
    int32_t bit_camera_obstacle; /* bit(c,o)  = bit_camera_obstacle + c*64 + o      (environment.py:752-755) */
    int32_t export_width;        /* doubles per environment in mate_engine_export_state */
    int32_t lut_capacity;        /* max knots per camera occlusion table */
    int32_t scalars_per_env;     /* floats per environment in the step scalar record (8) */
    int32_t specialised;         /* 1 = step kernels compiled for exactly this (Nc, Nt, No) run; 0 = generic kernels */
} mate_layout;

/* Per-step outputs (any pointer may be NULL to skip that output).
 *   scalars_dev: [N][8] f32 = camera_team_reward, target_team_reward, done, coverage_rate,
 *                real_coverage_rate, mean_transport_rate, num_delivered_cargoes,
 *                normalized target_team_reward   (environment.py:618-661)
 *   masks_dev:   [N][mask_words] u32 packed view masks + tracked bits (environment.py:1356-1388) */
typedef struct mate_step_io {
    const void *camera_actions_dev;   /* [N][Nc][2]  f32 or f64 (act_dtype) */
    const void *target_actions_dev;   /* [N][Nt][2] */
    int32_t act_dtype;
    const double *tape_camera_target_dev; /* [N][Nc][Nt] uniforms for the see-through draw, or NULL = Philox */
    const double *tape_goal_dev;          /* [N][Nt] uniforms for the goal choice, or NULL = Philox */
    void *camera_obs_dev;             /* [N][Nc][Dc] f32/f64 (obs_dtype) */
    void *target_obs_dev;             /* [N][Nt][Dt] */
    float *scalars_dev;
    uint32_t *masks_dev;
} mate_step_io;

typedef struct mate_engine mate_engine;

const char *mate_engine_last_error(void);
int mate_engine_abi_version(void);

/* MultiAgentTracking.__init__ (environment.py:330-562) for N environments on HIP device `device`.
 * RNG streams are keyed by (seed, first_env_index + i), so results do not depend on how a
 * global batch is sharded over GPUs.
 * Limits (MATE_EINVAL beyond them, never a silent fallback): at most 16 cameras, 16 targets, 64 obstacles (bit widths of
 * the packed records).  The occlusion-table build sorts 360 + 185 * obstacles rays per camera: in the 160 KiB LDS up
 * to 20 obstacles, in an HBM scratch slice per workgroup beyond (same code, slower resets; the reference's scenarios
 * use 0 or 9 obstacles with cameras, MATE-Navigation has 32 and no camera). */
int mate_engine_create(const mate_config *config, int64_t num_envs, int32_t device, uint64_t seed,
                       uint64_t first_env_index, mate_engine **out);
int mate_engine_destroy(mate_engine *engine);                               /* close(), environment.py:1192 */
int mate_engine_get_layout(const mate_engine *engine, mate_layout *out);
/* seed() (environment.py:1203-1227): installs the Philox key AND rewinds every counter that enters a counter word
 * (per-environment episode number, step tick), as the reference re-creates its RandomStates: after seed(s) the next
 * reset() and everything that follows depend on (s, global environment index) only, whatever ran before. */
int mate_engine_seed(mate_engine *engine, uint64_t seed);

/* reset() (environment.py:679-834) of every environment (env_mask_dev == NULL) or of those with a
 * non-zero byte in env_mask_dev[N].  Writes the initial observations/masks like a step does. */
int mate_engine_reset(mate_engine *engine, const uint8_t *env_mask_dev, const mate_step_io *io, void *stream);

/* reset() with every random draw of environment.py:679-834 on a tape (parity runs against the reference):
 * `tape_dev` [N][tape_len] uniforms in the reference's call order -- shuffles of the three entity lists, the
 * high-capacity choice, per placement attempt (camera: radius box, x, y, orientation index, viewing angle; obstacle:
 * radius, x, y; target: x, y), cargo pairs, goal choices of targets that spawn inside a warehouse, and per still
 * unloaded target a warehouse permutation + goal choice; how a uniform becomes a shuffle / choice / integer is stated
 * in oracle/mate_oracle.c above reset_impl (Fisher-Yates, a + int(u * n)).  io->tape_camera_target_dev, if set,
 * supplies the see-through uniforms of the first _update_view (environment.py:766).  `draws_used_dev` (optional,
 * [N] int32) receives the number of uniforms each environment consumed, -1 if its tape ran out.  tests/golden/
 * reset_*.npz hold such tapes recorded from the reference's own reset() together with the state it produced. */
int mate_engine_reset_tape(mate_engine *engine, const uint8_t *env_mask_dev, const mate_step_io *io,
                           const double *tape_dev, int32_t tape_len, int32_t *draws_used_dev, void *stream);

/* step() (environment.py:590-676).  auto_reset == 1: environments whose episode ended are reset in
 * the same call and their observation rows hold the first observation of the new episode (rewards/done
 * in `scalars_dev` still describe the finished step).  auto_reset == k > 1: batched resets -- a
 * finished environment idles (its scalar record reads done = 2, no new observation) until every k-th
 * call restarts all finished environments together, which amortises the reset latency (occlusion-table
 * build) when episodes end every step somewhere in the batch.  auto_reset == 0: the caller resets. */
int mate_engine_step(mate_engine *engine, const mate_step_io *io, int32_t auto_reset, void *stream);

/* Episode statistics for logging: `stats_dev` = 5 doubles in caller-owned device memory (or NULL to stop), to which
 * every later step / rollout launch adds, for each episode that ends in it: 1, the target team's episode reward
 * (environment.py:624), the episode length (:629), the final coverage_rate (:966) and num_delivered_cargoes.  This is
 * the record the sharded job all-gathers over RCCL; the engine only accumulates it, with a
 * handful of atomics per finished episode.  The caller zeroes / reads the buffer on its own streams. */
int mate_engine_set_episode_stats(mate_engine *engine, double *stats_dev);
/* ... and a snapshot of those 5 doubles into `dst_dev`, ordered on `stream` behind everything enqueued on it so far (one tiny launch):
 * the buffer a sharded job all-gathers while later launches go on accumulating (bench.py, StatsGather).  No reference counterpart:
 * the reference's trainers log episode returns on the host (SURVEY.md section 8e defines the record). */
int mate_engine_snapshot_episode_stats(mate_engine *engine, double *dst_dev, void *stream);

/* Graph-replayable stepping (the learner-in-the-loop flow: policy kernels write the joint actions into caller
 * buffers, step() consumes them, K such iterations are captured once in a HIP graph and replayed).  A step() launch
 * normally carries the step counter (the Philox tick) and the ping-pong index of the finished-episode lists as launch
 * arguments, which change at every step.  enable = k >= 1 moves both to device memory: the step kernels read them there
 * and the auto-reset launch that closes every interval of k steps advances them, so a whole interval (k step launches +
 * one auto-reset launch; k = 1: a (step, auto-reset) pair) has identical arguments every time and any number of
 * intervals may be captured (hipStreamBeginCapture on `stream`, or torch.cuda.graph) and replayed.  Results are
 * bit-identical to the host-counted flow with the same auto_reset.  While enabled only step() / step_random() /
 * step_greedy() / step_versus_greedy() with auto_reset = k, observe() and reset() are accepted (MATE_ESTATE otherwise) -- and
 * mate_engine_rollout_versus_greedy (FrameSkip in a graph): there k counts LAUNCHES, every launch of an interval has the same
 * number of frames K, and the auto-reset launch behind the k-th advances the counter by k * K.  enable == 0 (at an interval boundary)
 * drains `stream` and takes the counter back to the host.  The reference has no counterpart (environment.py:590 runs one
 * Python call per step); this is how its `for t in range(T): env.step(policy(obs))` loop is enqueued on a GPU. */
int mate_engine_device_tick(mate_engine *engine, int32_t enable, void *stream);

/* step() with the uniform random policy of SURVEY.md section 8d generated on-device
 * (camera U[-rot,rot] x U[-zoom,zoom], target U[-v,v]^2, Philox keyed by seed/env/tick);
 * io->*_actions_dev are ignored. */
int mate_engine_step_random(mate_engine *engine, const mate_step_io *io, int32_t auto_reset, void *stream);

/* `steps` consecutive step() calls under the on-device random policy fused into ONE launch (rollout
 * collection, the `for _ in range(T): env.step(...)` loop of examples/random.py).  Every io output
 * buffer is rollout-shaped: [steps][N][...] (row r*N + i = step r of environment i).  An environment
 * whose episode ends at step r stops there: its scalar rows of later steps carry done = 2 and its
 * observation rows are left untouched; with auto_reset it starts a new episode before the next call.
 * Those skipped slots are added to mate_engine_idle_steps.  auto_reset == k > 1 batches the restarts as step() does: a
 * finished environment idles through the following launches until every k-th call restarts all finished environments in
 * one reset launch (episodes that end every few steps somewhere in the batch, e.g. Greedy vs Greedy, otherwise pay one
 * latency-bound reset launch per rollout launch).  This is the fastest way to step: the records stay in LDS
 * for the whole launch and the waves of a SIMD take turns in issue priority (MATE_ROLLOUT_ROTATE=0 turns that off). */
int mate_engine_rollout_random(mate_engine *engine, const mate_step_io *io, int32_t steps, int32_t auto_reset, void *stream);

/* On-device rule-based policies: the reference's GreedyCameraAgent / GreedyTargetAgent
 * (mate/agents/greedy.py:13-227, 229-365) for every agent of every environment, acting on the same
 * partial observations (own state, opponents gated by the view masks of the previous step, teammates'
 * messages).  mate_engine_policy_enable() must precede the reset()/step() whose view they first act on.  Any scenario the
 * engine takes (up to 16 cameras and 16 targets): the camera agents' message exchange runs one lane per sender-recipient pair,
 * in as many rounds of 64 pairs as the cameras need; the fused rollouts need the workgroup's four environments -- step
 * records + agents' memory -- to fit the 160 KiB LDS (MATE_EINVAL otherwise, mate_engine_step_greedy still works).
 * mate_engine_step_greedy() = group_step of both teams (observe, two-phase message exchange, act;
 * mate/wrappers/single_team.py:79-92) + step().  `tape` (device arrays, any member NULL = Philox):
 * recorded draws of the agents, for parity runs.  (mate_engine_policy_enable also tabulates the camera agents' 20-iteration
 * zoom solve, greedy.py:139-145 -- a function of one scalar -- with the reference's own iteration: 225 KB, read with cubic
 * interpolation to 1.5e-13 degrees; the agents' memory, joint actions and a copy of the view masks are allocated there too.) */
typedef struct mate_policy_tape {
    const double *camera_resample_u_dev;     /* [N][Nc]      Bernoulli(0.1) uniform when no target is remembered (greedy.py:93) */
    const double *camera_sample_u_dev;       /* [N][Nc][2]   action_space.sample() uniforms (greedy.py:94) */
    const int32_t *camera_delay_dev;         /* [N][Nc][Nc]  randint(6, 50) per sent message sender->recipient (greedy.py:184) */
    const double *target_choice_u_dev;       /* [N][Nt]      choice among non-empty warehouses (greedy.py:298) */
    const double *target_resample_u_dev;     /* [N][Nt]      Bernoulli(prob) uniform (greedy.py:316) */
    const double *target_sample_u_dev;       /* [N][Nt][2]   noise sample uniforms (greedy.py:317) */
    const double *target_reset_sample_u_dev; /* [N][Nt][2]   initial noise at agent.reset (greedy.py:277) */
} mate_policy_tape;
int mate_engine_policy_enable(mate_engine *engine);
int mate_engine_step_greedy(mate_engine *engine, const mate_step_io *io, const mate_policy_tape *tape,
                            int32_t auto_reset, void *stream);
/* MultiCamera / MultiTarget (mate/wrappers/single_team.py:180-306, SingleTeamMultiAgent.step :245-264): the caller -- the
 * learner of examples/ippo|mappo|qmix|... -- plays ONE team, the on-device greedy agents play the other:
 * `group_step(env, opponent_agents, ...)` + `env.step((action, opponent_joint_action))` -- ONE launch (step_greedy_kernel: the opponents'
 * agents, then the step) unless a policy tape, a step tape, a fused observation transform / team mode, f64 observations or a missing output
 * asks for the two-launch form.  Only the OPPONENTS' agents act, as in the reference's wrapper (which holds no agents for the learner's team):
 * the caller's team's agent memory is left as it is, and a team's agent.reset(observation) runs at its own first acting call of an episode.  `team` is the
 * CALLER's team; io->camera_actions_dev (MATE_TEAM_CAMERA) or io->target_actions_dev (MATE_TEAM_TARGET) holds its joint
 * action in the encoding io->act_dtype names (f32 / f64 pairs, or grid indices with that team's *_DISCRETE bit); the other
 * action pointer is ignored.  The opponents observe, exchange messages and act exactly as in mate_engine_step_greedy
 * (their draws come from the same Philox streams / `tape`), so feeding the greedy agents' own recorded joint action for
 * `team` reproduces the step_greedy trajectory bit for bit (tests/test_gpu_policies.py). */
enum { MATE_TEAM_CAMERA = 0, MATE_TEAM_TARGET = 1 };           /* mate/utils.py Team */
int mate_engine_step_versus_greedy(mate_engine *engine, int32_t team, const mate_step_io *io, const mate_policy_tape *tape,
                                   int32_t auto_reset, void *stream);
/* `steps` consecutive (agents act, environment steps) iterations of GreedyCameraAgent vs GreedyTargetAgent fused into ONE
 * launch: mate.group_step + env.step of the evaluation loop (mate/evaluate.py:104-139, agents/greedy.py), with the
 * environment records, the agents' memory and the view masks resident in LDS.  Outputs are rollout-shaped like
 * mate_engine_rollout_random ([steps][N][...]); observations and scalars are required.  An environment whose episode ends
 * stops there (done = 2 in its later scalar rows, counted by mate_engine_idle_steps) and, with auto_reset, starts a new
 * episode before the next call.  Philox draws only (no policy tape).  Bit-identical to `steps` calls of
 * mate_engine_step_greedy. */
/* auto_reset == MATE_RESET_PIPELINED: restarts taken off the critical path.  Greedy-vs-Greedy episodes last ~1.2 k steps, so a few
 * hundred of 8192 environments finish in every launch and their reset -- placement, one occlusion table per camera, first view:
 * three latency-bound launches, ~0.25 ms -- otherwise sits between two rollout launches.  Here the reset of what launch n
 * finished is enqueued on a stream of the engine's own behind launch n and runs UNDER launch n + 1; a restarted environment joins
 * launch n + 2 (its `done` word carries a hand-over tag: no launch ever steps or stores an environment a concurrent reset owns,
 * so results do not depend on timing -- the same calls with MATE_PIPELINED_SERIAL=1, which runs the resets on the caller's
 * stream, give the same bytes).  A finished environment idles through the rest of its launch and all of the next one (scalar
 * rows done = 2, counted by mate_engine_idle_steps).  Any other entry point of the handle first waits for the resets in flight
 * and turns the tags back into plain live environments.
 * auto_reset = -m (m > 1): ONE such restart launch behind every m-th rollout launch (short launches -- a learner's FrameSkip actions --
 * whose restart group is longer than a launch): what finishes in interval i of m launches idles through i + 1 and is live again in
 * the first launch of i + 2; leaving the mode inside an interval restarts what it had listed.  (Measured on FrameSkip(5) launches of
 * MATE-4v8-9 x 4096 / 16 384: 65.5 against 66.3 us per launch and 1.3 % more idle slots -- no gain: the launch fills its registers'
 * worth of every SIMD and the restart's workgroups wait for its tail either way.  tools/archive/frameskip_pipelined_probe.py) */
#define MATE_RESET_PIPELINED (-1)
int mate_engine_rollout_greedy(mate_engine *engine, const mate_step_io *io, int32_t steps, int32_t auto_reset, void *stream);
/* FrameSkip(frame_skip = steps) over MultiCamera / MultiTarget (examples/utils/wrappers.py:301-323: the same action for
 * `frame_skip` env.step calls; every example trainer's make_env applies it last) in ONE launch: the caller's `team` repeats
 * the joint action of io (as in mate_engine_step_versus_greedy) for `steps` frames, the greedy opponents act anew on every
 * frame.  Outputs are rollout-shaped; the wrapper's summed reward is the column sum of the scalar rows (rows with
 * done = 2 are zero), its observation the last row with done != 2.  Bit-identical to `steps` calls of
 * mate_engine_step_versus_greedy with the same action.  Graph-replayable under mate_engine_device_tick (see there). */
int mate_engine_rollout_versus_greedy(mate_engine *engine, int32_t team, const mate_step_io *io, int32_t steps,
                                      int32_t auto_reset, void *stream);

/* copies the joint actions of the last step_greedy into caller buffers [N][Nc][2] / [N][Nt][2] f64 (either may be NULL): what the step
 * consumed -- with the Heuristic target opponent (below) the FINAL target actions.  mate_engine_policy_greedy_target_actions: the Greedy
 * target agents' joint action of the same step, ahead of the drift (the same array while the opponent is Greedy). */
int mate_engine_policy_actions(mate_engine *engine, double *camera_actions_dev, double *target_actions_dev, void *stream);
int mate_engine_policy_greedy_target_actions(mate_engine *engine, double *target_actions_dev, void *stream);

/* Which scripted agent plays the TARGET team where the engine plays it (the reference's opponent_agent_factory of
 * camera configurations under examples/, mate.evaluate's --target-agent):
 *   MATE_OPPONENT_GREEDY     GreedyTargetAgent (mate/agents/greedy.py:229-365), the default; nothing changes while it is selected
 *   MATE_OPPONENT_HEURISTIC  HeuristicTargetAgent (mate/agents/heuristic.py:290-337): the Greedy target's action, then a drift away from the
 *                            incentre of the nearest camera sector the target senses and lies in or near -- reached through the sector's SIGNED
 *                            angle test, as the reference writes it (:308-311) --, applied where it does not oppose the action (:332-335).
 *                            The agent draws nothing, remembers nothing and sends nothing of its own: ONE launch (csrc/opponent_rows.hpp) over the
 *                            Greedy agents' joint action, out of place, into an engine-owned [N][Nt][2] f64 buffer allocated at the first switch.
 * Needs mate_engine_policy_enable (MATE_ESTATE); may change at any call boundary (waits for the handle's launches; no agent memory to migrate).
 * While Heuristic is selected:
 *   - mate_engine_step_greedy, mate_engine_step_versus_greedy(MATE_TEAM_CAMERA) and mate_engine_step_selected take the TWO-launch form with the
 *     drift launch in it: [executor,] agents' launch, drift launch, stepping launch reading the final buffer, then what follows a step as before.
 *     The drift launch has identical arguments at every call, allocates nothing and does not synchronise: capturable under
 *     mate_engine_device_tick, with tapes or Philox draws.  Environments the agents' launch skips (done = 2 under a batched restart) keep
 *     their Greedy row; a scenario without cameras makes it a copy (bit-identical results to the Greedy opponent).
 *   - mate_engine_step_versus_greedy(MATE_TEAM_TARGET) and mate_engine_rollout_versus_greedy(MATE_TEAM_TARGET) are unaffected: the caller plays
 *     the targets.
 *   - mate_engine_rollout_greedy and mate_engine_rollout_versus_greedy(MATE_TEAM_CAMERA) return MATE_ESTATE: the fused K-frame kernels hold the
 *     Greedy agents.  (FrameSkip against this opponent is K per-step calls in one graph.)
 *   - mate_engine_set_obs_mode with a non-plain TARGET team mode returns MATE_EINVAL, and selecting Heuristic under such a mode does: the
 *     opponents' `sensed` is the flag column of their plain rows.
 * MATE_EINVAL: an unknown opponent. */
enum { MATE_OPPONENT_GREEDY = 0, MATE_OPPONENT_HEURISTIC = 1 };
int mate_engine_set_target_opponent(mate_engine *engine, int32_t opponent);

/* Which scripted agent plays the CAMERA team where the engine plays it (the reference's opponent_agent_factory of target configurations under
 * examples/, mate.evaluate's --camera-agent):
 *   MATE_OPPONENT_GREEDY     GreedyCameraAgent (mate/agents/greedy.py:13-227), the default; nothing changes while it is selected
 *   MATE_OPPONENT_HEURISTIC  HeuristicCameraAgent (mate/agents/heuristic.py:17-287): camera 0 collects the team's observations, scores 756 poses
 *                            per camera against a table over the sensed targets in range, tries 32 orders of greedy assignment and sends
 *                            every camera with a target in range the winning pose as its goal; a camera without one repeats or, with
 *                            probability 0.1, re-samples its action.  ONE launch, heuristic_camera_kernel (csrc/opponent_rows.hpp: semantics,
 *                            draws, mapping), into engine-owned buffers allocated at the first switch: the joint action [N][Nc][2] f64 the
 *                            stepping launch reads, prev_action, the goals [N][Nc][2] (NaN where none) and their state indices [N][Nc] (-1).
 * Needs mate_engine_policy_enable (MATE_ESTATE) and, for Heuristic in a scenario with cameras, the tables (MATE_ESTATE):
 *   mate_engine_heuristic_camera_tables   state_mesh [756][3], coord_grid [2952][2], scores [2952][756] f64 HOST arrays, copied once to the
 *                                         device (MATE_EINVAL: a null table).  The library has no generator: mate_amd/heuristic_tables.py is
 *                                         the one the Python host uses; one set per (round(max_sight_range, 8), round(min_viewing_angle, 8)).
 *   mate_engine_heuristic_camera_tape     permutations_dev [N][32][Nc] int8 recorded permutations of the controller (NULL: Philox draws), and
 *                                         record_dev [N][32][Nc] int8 that receives the permutations every launch used (NULL: nothing is
 *                                         stored).  Both hold until replaced.  The Bernoulli and sample uniforms of a parity run come through
 *                                         mate_policy_tape.camera_resample_u_dev / camera_sample_u_dev, as for the Greedy cameras;
 *                                         camera_delay_dev is ignored (these agents' messages arrive within the step).
 *   mate_engine_heuristic_camera_goals    copies the last launch's goals [N][Nc][2] f64 and state indices [N][Nc] i32 out (either may be NULL).
 * The opponent may change at any call boundary (the setter waits for the handle's launches).  Switching to Heuristic zeroes prev_action and makes
 * the agents' reset run at their first acting call; switching back marks the Greedy camera agents -- which sat out meanwhile -- for THEIR reset
 * (prev_action, memory, message delays) at their next acting call, if a Heuristic launch ran in between (else their memory is current and stays).
 * While Heuristic is selected:
 *   - mate_engine_step_greedy takes the TWO-launch form: the agents' launch with the camera team not acting, [the drift launch,] the Heuristic
 *     cameras' launch, the stepping launch reading its buffer.  mate_engine_step_versus_greedy(MATE_TEAM_TARGET) runs no agents' launch (nobody
 *     of the Greedy pair acts): the Heuristic cameras' launch, then the step.  Identical arguments at every call, no allocation, no
 *     synchronisation: capturable under mate_engine_device_tick.  An environment idling under a batched restart (done = 2) is skipped: it keeps
 *     its rows and its prev_action.  mate_engine_policy_actions reports the final camera action.
 *   - mate_engine_step_versus_greedy(MATE_TEAM_CAMERA), mate_engine_step_selected and mate_engine_rollout_versus_greedy(MATE_TEAM_CAMERA) are
 *     unaffected: the caller (or the executor) plays the cameras.
 *   - mate_engine_rollout_greedy and mate_engine_rollout_versus_greedy(MATE_TEAM_TARGET) return MATE_ESTATE: the fused K-frame kernels hold the
 *     Greedy agents.  (FrameSkip against this opponent is K per-step calls in one graph.)
 *   - mate_engine_set_obs_mode with a non-plain CAMERA team mode returns MATE_EINVAL, and selecting Heuristic under such a mode does.
 * A scenario without cameras makes the selection a no-op (bit-identical to Greedy).  Both heuristic opponents may be on together.
 * MATE_EINVAL: an unknown opponent. */
int mate_engine_set_camera_opponent(mate_engine *engine, int32_t opponent);
int mate_engine_heuristic_camera_tables(mate_engine *engine, const double *state_mesh, const double *coord_grid, const double *scores);
int mate_engine_heuristic_camera_tape(mate_engine *engine, const int8_t *permutations_dev, int8_t *record_dev);
int mate_engine_heuristic_camera_goals(mate_engine *engine, double *goals_dev, int32_t *indices_dev, void *stream);

/* Opponent MIXTURES: per environment and EPISODE, which scripted agent plays a team the engine plays (the reference's MixtureCameraAgent /
 * MixtureTargetAgent, mate/agents/mixture.py -- the opponents PSRO trains against; spawn() seeds a team's agents alike, so the whole team plays
 * one candidate per episode), over five kinds:
 *   MATE_SCRIPTED_GREEDY / _HEURISTIC   the two pairs above
 *   MATE_SCRIPTED_NAIVE                 NaiveCameraAgent / NaiveTargetAgent (mate/agents/naive.py)
 *   MATE_SCRIPTED_RANDOM                RandomCameraAgent / RandomTargetAgent (mate/agents/random.py): a uniform action held for random_frame_skip
 *                                       acting calls -- NOT mate_engine_step_random, which draws anew on every frame
 *   MATE_SCRIPTED_EXTERNAL              rows the caller writes, before each stepping call and for every environment, into the engine-owned
 *                                       [N][n][2] f64 buffer mate_engine_scripted_external returns (a learned population member the host
 *                                       evaluates on the batch; the device picks the rows of the environments that drew it)
 * ONE more launch, scripted_opponent_kernel (csrc/scripted_rows.hpp: semantics, draws, mapping), behind the agents' launch, the Heuristic cameras'
 * launch and the drift launch and ahead of the stepping launch of mate_engine_step_greedy, mate_engine_step_versus_greedy and
 * mate_engine_step_selected (the two-launch form): at a team's first acting call of an episode it draws the team's kind,
 *   k = searchsorted(cumsum(w / sum w), u, side='right') over the candidates with positive weight in the order given,
 * computes the Naive or Random agents where the kind asks for them, and writes the team's FINAL joint action -- the Greedy row, the Heuristic
 * row, the external row or its own -- into an engine-owned buffer the stepping launch reads.  mate_engine_policy_actions reports those rows.
 * Identical arguments at every call, no allocation, no synchronisation: capturable under mate_engine_device_tick.  The Greedy agents' launch
 * (Greedy or Heuristic targets; Greedy cameras) and the Heuristic cameras' launch run only where some candidate with positive weight needs
 * them, and then for EVERY environment, whatever its choice.  An environment idling under a batched restart keeps memory, choice and final row.
 *   mate_engine_set_opponent_mixture   kinds[count], weights[count] (NULL: all 1).  count = 0 clears the team's mixture (the plain selection it
 *       replaced returns; the Greedy agents of the team reset at their next acting call).  ONE candidate of kind Greedy or Heuristic is exactly
 *       that plain selection: no launch, the same bytes.  Installing or changing a mixture makes the team's reset -- and draw -- run at its next
 *       acting call; Greedy agents that sat out under the old mixture and act under the new one reset at that call too.  While a mixture is installed for a team, that team's mate_engine_set_target_opponent / mate_engine_set_camera_opponent
 *       returns MATE_ESTATE, and while it is anything but {Greedy} the fused K-frame launches that would play the team (mate_engine_rollout_greedy,
 *       mate_engine_rollout_versus_greedy of the other team) return MATE_ESTATE: FrameSkip is K per-step calls in one graph.
 *       MATE_EINVAL: a team that is neither, an unknown or repeated kind, more than five candidates, a negative or non-finite weight, all weights
 *       zero, random_frame_skip < 1, a Heuristic candidate under a non-plain observation mode of the team.  MATE_ESTATE: before
 *       mate_engine_policy_enable; a Heuristic camera candidate without mate_engine_heuristic_camera_tables.  A refused call changes nothing.
 *   mate_engine_scripted_tape          recorded draws (the four tape members; any of them NULL: Philox for that member) and a record of the draws
 *       used (the four record_ members, the same shapes; any of them NULL: not stored), installed with ONE call.  camera_u_dev [N][Nc][2] (Naive: [0]; Random: both), target_u_dev [N][Nt][3] (the binomial u, the two sample uniforms;
 *       Random: the latter two), target_reset_dev [N][Nt][4] (the two sample uniforms of prev_noise, goal, inc, as doubles), choice_dev [2][N]
 *       int32 kinds by team (-1, or a kind outside the mixture: draw).  The record's doubles read NaN where nothing was drawn; its choice rows
 *       receive the kind each team under a mixture holds.  Both hold until replaced.  MATE_EINVAL: record_camera_u_dev or record_target_reset_dev not aligned to 16 bytes (the
 *       launch stores pairs of doubles there), any other buffer not aligned to its element size.
 *   mate_engine_scripted_memory        copies a team's memory out (device buffers, any may be NULL): choice [N] (the kind; -1 before the first
 *       draw), goal [N][Nt], inc [N][Nt], prev_noise [N][Nt][2] (the Naive targets'; ignored for the cameras), prev_action [N][n][2] and counter
 *       [N] (the Random agents').  MATE_ESTATE: no mixture with a launch has been installed for the team.
 *   mate_engine_scripted_external      the team's [N][n][2] f64 external buffer (MATE_ESTATE as above).
 *   mate_engine_scripted_rows          copies one SOURCE of the team's final rows out, [N][n][2] f64 as the last launch read it: kind Greedy (the
 *       Greedy agents' joint action), Heuristic (MATE_ESTATE while the team has no Heuristic candidate) or External; MATE_EINVAL for Naive and
 *       Random, whose rows exist only as final rows (mate_engine_policy_actions). */
enum { MATE_SCRIPTED_GREEDY = 0, MATE_SCRIPTED_HEURISTIC = 1, MATE_SCRIPTED_NAIVE = 2, MATE_SCRIPTED_RANDOM = 3, MATE_SCRIPTED_EXTERNAL = 4 };
int mate_engine_set_opponent_mixture(mate_engine *engine, int32_t team, const int32_t *kinds, const double *weights, int32_t count,
                                     int32_t random_frame_skip);
int mate_engine_scripted_tape(mate_engine *engine, const double *camera_u_dev, const double *target_u_dev, const double *target_reset_dev,
                              const int32_t *choice_dev, double *record_camera_u_dev, double *record_target_u_dev,
                              double *record_target_reset_dev, int32_t *record_choice_dev);
int mate_engine_scripted_memory(mate_engine *engine, int32_t team, int32_t *choice_dev, int32_t *goal_dev, int32_t *inc_dev,
                                double *prev_noise_dev, double *prev_action_dev, int32_t *counter_dev, void *stream);
int mate_engine_scripted_external(mate_engine *engine, int32_t team, double **rows_dev);
int mate_engine_scripted_rows(mate_engine *engine, int32_t team, int32_t kind, double *rows_dev, void *stream);

/* joint_observation() (environment.py:908-983) without advancing the simulation: recomputes
 * the view masks from the current state (see-through draws from io tape or Philox) and packs. */
int mate_engine_observe(mate_engine *engine, const mate_step_io *io, void *stream);

/* Fuse the reference's observation post-processing wrappers into the packer (no second pass over the
 * observation bytes): relative != 0 = RelativeCoordinates (mate/agents/utils.py:40-94: coordinates of
 * warehouses and of visible entities minus the observing agent's own location); scale/bias per column
 * ([camera_obs_dim] / [target_obs_dim], host arrays, NULL = identity) = any affine per-column map, e.g.
 * RescaledObservation (utils.py:97-137).  out = ((value - own) if visible else 0) * scale + bias.
 * All NULL / 0 restores the plain observations. */
int mate_engine_set_obs_transform(mate_engine *engine, int32_t relative, const double *camera_scale,
                                  const double *camera_bias, const double *target_scale, const double *target_bias);

/* Team observation modes, fused into the packer as well: 0 plain; 1 = EnhancedObservation
 * (mate/wrappers/enhanced_observation.py:72-126: every opponent / obstacle / teammate block visible, targets see
 * the true emptiness of all warehouses); 2 = SharedFieldOfView (mate/wrappers/shared_field_of_view.py:72-148:
 * an opponent or obstacle is visible to the whole team when any member sees it, teammates always visible,
 * targets share their empty-warehouse knowledge).  The exported view masks are not affected, like in the
 * reference (the wrappers only rewrite observations). */
#define MATE_OBS_PLAIN 0
#define MATE_OBS_ENHANCED 1
#define MATE_OBS_SHARED 2
int mate_engine_set_obs_mode(mate_engine *engine, int32_t camera_team_mode, int32_t target_team_mode);

/* Normalised action grids for discrete joint actions (host arrays [n][2], copied; n = 0 / NULL removes one):
 * continuous action = action_high * grid[index], with action_high = (rotation_step, zooming_step) for a camera
 * and the target's own step size for a target (discrete_action_spaces.py:71-73, 161-163, 177-179).  Indices
 * outside [0, n) are clamped on the device; the Python boundary raises like the reference's assert. */
int mate_engine_set_action_grids(mate_engine *engine, const double *camera_grid, int32_t num_camera_actions,
                                 const double *target_grid, int32_t num_target_actions);

/* Canonical f64 export / import of the whole simulation state, [N][export_width] doubles
 * (layout documented in DESIGN.md; used by state(), the attribute views and the parity tests). */
int mate_engine_export_state(mate_engine *engine, double *dst_dev, void *stream);
int mate_engine_import_state(mate_engine *engine, const double *src_dev, void *stream);

/* Global state rows: MultiAgentTracking.state() (environment.py:894-906) of every environment, written on the device -- what the
 * reference's centralised-critic trainers (MAPPO, MADDPG, QMIX-style mixers, I2C, TarMAC) read after every reset() and step()
 * (examples/utils/wrappers.py:170-225).  One row of S = mate_layout.state_dim reals per environment, in the reference's order:
 *   preserved_data (13; element 3, the agent index of an observation row, is 0) | per camera state(private=True) (9) |
 *   per target state(private=True) (14) | per obstacle state() (3) | freights (Nt) | bounties (Nt) | remaining_cargoes (16)
 * `out_dtype`: MATE_OBS_F32 or MATE_OBS_F64, whatever the engine's obs_dtype is.  A raw row's camera / target blocks are bit-identical
 * to elements [13:22] / [13:27] of that agent's plain observation row of the same type.  `scale` / `bias` (host arrays [S], both or
 * neither): an affine map per element, out = value * scale + bias (no fused multiply-add), e.g. mate.normalize_observation(state,
 * env.state_space) (mate/agents/utils.py:97-127: minus `low` where bounded below, then 2 x / (high - low) - 1 where bounded on both
 * sides; what examples/utils/wrappers.py:188, 225 apply) -- the tables are copied.  The output is one densely packed [N][S] array in
 * caller-owned device memory, 16-byte aligned (rows themselves are in general not: S = 81, 111, 193, 253 ...).
 *
 * mate_engine_enable_state_rows attaches `dst_dev` (NULL detaches; MATE_ESTATE before the first reset / import_state).  While
 * attached, every call that leaves new records behind -- reset / reset_tape (masked ones included), step, step_random, step_greedy,
 * step_versus_greedy, observe, import_state, rollout_random / rollout_greedy / rollout_versus_greedy -- enqueues ONE more launch, the
 * last of the call on the call's stream, that rewrites all N rows.  "Last" is behind the auto-reset launch where the call has one:
 * with auto_reset = 1 a restarted environment's state row and observation rows both show the new episode while the scalar record keeps
 * describing the finished step; under a batched restart (auto_reset = k > 1) an idling environment's row keeps its terminal state
 * until the restart launch.  A fused rollout leaves the state after its LAST frame only (what FrameSkip over a centralised-training
 * wrapper hands the learner).  The launch is capturable -- no host synchronisation, no allocation, the same arguments at every call
 * -- so an interval captured under mate_engine_device_tick contains it and a replay refreshes the rows.  Enabling itself writes
 * nothing (follow it with mate_engine_state_rows or any of the calls above) and waits for the handle's launches in flight.
 * Pipelined restarts (auto_reset = MATE_RESET_PIPELINED / -m of mate_engine_rollout_greedy) rewrite records on the engine's side
 * stream under the caller's next launches, where a reader of the records would race with them: with rows attached that mode
 * returns MATE_ESTATE (it is a Greedy-vs-Greedy measurement flow without a learner).
 *
 * mate_engine_state_rows: one such launch on `stream` into any buffer, nothing attached (the on-demand form, as
 * mate_engine_export_state is for the checkpoint).  With a map that differs from the previous on-demand call's it first waits for
 * the handle's launches in flight and uploads the table; the same map again costs neither.
 * MATE_EINVAL: NULL engine, an out_dtype other than the two, one of scale / bias without the other, a misaligned buffer (NULL in the
 * on-demand form); MATE_ESTATE: before the first reset / import_state. */
int mate_engine_enable_state_rows(mate_engine *engine, void *dst_dev, int32_t out_dtype, const double *scale, const double *bias);
int mate_engine_state_rows(mate_engine *engine, void *dst_dev, int32_t out_dtype, const double *scale, const double *bias, void *stream);

/* Shaped per-agent rewards: the reference's AuxiliaryCameraRewards (mate/wrappers/auxiliary_camera_rewards.py:110-176) and
 * AuxiliaryTargetRewards (mate/wrappers/auxiliary_target_rewards.py:128-203) -- the last wrapper of every example trainer's chain
 * (examples/<algorithm>/camera/config.py, .../target/config.py) -- with one coefficient per term, written on the device by one launch attached to the engine.
 * Per agent: the sum, in the order below, of coefficient * term over the terms whose coefficient is not exactly 0 (no fused
 * multiply-add), then the team's reduction, the reduced value written to every agent's slot.
 *   camera terms [7]:  raw_reward (scalar column 0), coverage_rate, real_coverage_rate, mean_transport_rate (columns 3, 4, 5: the f32
 *                      step record widened to f64), soft_coverage_score (the per-camera score of mate_engine_soft_coverage),
 *                      num_tracked (bits of camera_target_view_mask), baseline (1)
 *   target terms [10]: raw_reward (column 1), coverage_rate, real_coverage_rate, mean_transport_rate, normalized_goal_distance
 *                      (distance to the rim of the goal warehouse, without a goal of the nearest non-empty one, with all of them empty
 *                      half the terrain; over the terrain width), sparse_delivery (the goal differs from the one the previous launch
 *                      saw, that one was >= 0, same episode: environment.py:1320-1322), soft_coverage_score (the score matrix summed over
 *                      the cameras that see the target, else tanh of its maximum), is_tracked, is_colliding, baseline (1)
 * `*_rows_dev`: [N][Nc] / [N][Nt] of `out_dtype` (MATE_OBS_F32 / MATE_OBS_F64, whatever the engine's obs_dtype is), caller-owned; a NULL
 * team is absent.  `*_terms_dev` (optional, with that team's rows): [N][Nc][7] / [N][Nt][10] f64, every term of the last launch (the
 * reference's info['auxiliary_reward_<key>']).  `*_coefficients_dev`: DEVICE arrays [7] / [10] f64 the launch reads every time -- a
 * training-progress schedule rewrites them in place, between the replays of a captured graph too.  `soft_coverage` != 0: the
 * soft_coverage_score terms exist -- every reward launch is preceded by the soft-coverage launch into engine-owned buffers (needs
 * cameras and mate_engine_enable_outer_boundary); without it that term reads NaN, which a non-zero coefficient carries into the row.
 * `accumulate` != 0: rows += shaped instead of rows = shaped (FrameSkip's sum over per-step launches; the caller zeroes the rows when
 * it consumes them).
 *
 * While attached (NULL `config` detaches):
 *   step / step_random / step_greedy / step_versus_greedy and the fused rollout_* (there: state and scalar / mask rows of the launch's
 *   LAST frame, sparse_delivery against the previous reward launch) enqueue the reward launch BEHIND the stepping launch and AHEAD of the
 *   restart of finished episodes: the rows describe the step `scalars_dev` describes, the terminal one included, under every
 *   auto_reset.  These calls then need io->scalars_dev and io->masks_dev (MATE_EINVAL otherwise).  An environment whose scalar record
 *   says done = 2 (idling under a batched restart) contributes nothing: zero rows, nothing added when accumulating.
 *   Behind every restart launch the engine issues (immediate, batched, a flushed interval) and behind reset / reset_tape / import_state
 *   one more launch refreshes only the goals / episode the next sparse_delivery is measured against.  observe: no launch.
 *   With state rows attached too: stepping launch, reward launch, restart, refresh, state rows last.
 *   Pipelined restarts (MATE_RESET_PIPELINED / -m) return MATE_ESTATE, as with state rows.
 * No allocation, no synchronisation, the same arguments at every call: an interval captured under mate_engine_device_tick contains the
 * launches.  Enabling itself waits for the handle's launches in flight and runs one refresh launch.
 * MATE_ESTATE: before the first reset / import_state; soft_coverage without the outer boundary.  MATE_EINVAL: no team, a camera team
 * (or soft_coverage) in a scenario without cameras, rows without coefficients, terms without rows, a misaligned buffer, an unknown
 * out_dtype or reduction (MATE_REDUCE_MIN is the camera wrapper's alone). */
enum { MATE_REDUCE_NONE = 0, MATE_REDUCE_MEAN = 1, MATE_REDUCE_SUM = 2, MATE_REDUCE_MAX = 3, MATE_REDUCE_MIN = 4 };
#define MATE_CAMERA_REWARD_TERMS 7
#define MATE_TARGET_REWARD_TERMS 10
typedef struct mate_reward_rows {
    void *camera_rows_dev, *target_rows_dev;
    double *camera_terms_dev, *target_terms_dev;
    int32_t out_dtype;
    int32_t camera_reduction, target_reduction;
    int32_t accumulate;
    int32_t soft_coverage;
    const double *camera_coefficients_dev, *target_coefficients_dev;
} mate_reward_rows;
int mate_engine_enable_reward_rows(mate_engine *engine, const mate_reward_rows *config);

/* Target-selection camera actions: the per-frame part of the reference's HierarchicalCamera wrapper (examples/hrl/wrappers.py), the
 * wrapper every hierarchical camera trainer (examples/hrl/<algorithm>/camera) goes through.  The learner emits a selection of targets per camera;
 * a fixed executor (HierarchicalCamera.track, wrappers.py:183-220) turns it into the camera team's continuous joint action on EVERY
 * frame, from the camera's true state, the selected targets' true positions and the camera's view of the previous frame.  Attached
 * launches of one kernel (csrc/selection_rows.hpp); no stepping kernel changes.
 *   mode MATE_SELECTION_SINGLE: selection_dev [N][Nc] int32, an index in [0, Nt]; Nt selects nothing (the wrapper's index2onehot)
 *   mode MATE_SELECTION_MULTI:  selection_dev [N][Nc] uint32, bit t = target t selected (Nt <= 16)
 * read at every mate_engine_step_selected; values are not validated (bits beyond Nt are ignored, an index outside [0, Nt) selects nothing).
 * Optional outputs, caller-owned: metrics_dev [N][Nc][4] f64 = num_selected_targets, num_valid_selected_targets,
 * num_invalid_selected_targets, invalid_target_selection_rate (= invalid / max(1, selected)) of wrappers.py:120-136, against the view of
 * the step that has just run; frames_dev [N] int32 = frames that contributed; action_mask_dev = action_mask() (wrappers.py:166-175) of
 * the observation the learner sees next: [N][Nc][2 Nt] u8 with the even entries 1 (multi) / [N][Nc][Nt + 1] u8 with the last entry 1.
 * flags: MATE_SELECTION_ACCUMULATE -- metrics += and frames += 1 per frame instead of = (FrameSkip's mean is metrics / frames; the caller
 * zeroes both when it consumes them); MATE_SELECTION_ACT_F32 -- the engine-owned joint action is f32 pairs (default f64).
 * An environment whose scalar record says done = 2 (idling under a batched restart) contributes nothing: zero rows and count, or, accumulating,
 * nothing added.  "View" is the opponent-flag column of the camera rows: the camera_target_view_mask bits, their OR over the cameras under
 * MATE_OBS_SHARED, all ones under MATE_OBS_ENHANCED (camera team mode).
 *
 * mate_engine_step_selected enqueues, in this order: the executor; exactly what mate_engine_step_versus_greedy(MATE_TEAM_CAMERA) enqueues,
 * reading the engine-owned joint action (io->camera_actions_dev is ignored); the reward launch when reward rows are attached; the metrics
 * launch; the restart of finished episodes; the action-mask launch; state rows last.  The executor reads the engine's own mask words as the
 * previous step, reset or restart launch left them: a restarted environment acts on its new episode's first view.  Every check, and
 * whatever the stepping flow enqueues ahead of its launch, precedes the executor: a rejected call leaves the action buffer alone.  While
 * selection is attached the action-mask launch also follows mate_engine_reset / _reset_tape / _observe and the other stepping calls
 * (ahead of state rows), whenever the engine's mask words are current; mate_engine_enable_selection writes it once and returns with it
 * complete.  io->scalars_dev is required.  No allocation, no synchronisation, identical arguments at every call: capturable under mate_engine_device_tick.
 * MATE_ESTATE: before mate_engine_policy_enable / the first reset; auto_reset = MATE_RESET_PIPELINED (and the pipelined rollouts while
 * attached); view masks older than the records (a fused random rollout restarted episodes, import_state: observe() first).
 * MATE_EINVAL: a null selection buffer, an unknown mode or flag, no cameras, a misaligned buffer.
 * mate_engine_selection_actions: the engine-owned joint action [N][Nc][2] and its MATE_ACT_F32 / MATE_ACT_F64 type (what the last
 * mate_engine_step_selected executed). */
enum { MATE_SELECTION_SINGLE = 0, MATE_SELECTION_MULTI = 1 };
enum { MATE_SELECTION_ACCUMULATE = 1, MATE_SELECTION_ACT_F32 = 2 };
#define MATE_SELECTION_METRICS 4
int mate_engine_enable_selection(mate_engine *engine, int32_t mode, const void *selection_dev, double *metrics_dev, int32_t *frames_dev,
                                 uint8_t *action_mask_dev, int32_t flags);
int mate_engine_disable_selection(mate_engine *engine);
int mate_engine_selection_actions(mate_engine *engine, void **actions_dev, int32_t *act_dtype);
int mate_engine_step_selected(mate_engine *engine, const mate_step_io *io, const mate_policy_tape *tape, int32_t auto_reset, void *stream);

/* FrameSkip fragments: what the reference's FrameSkip wrapper (examples/utils/wrappers.py:301-323) at the end of every example trainer's chain
 *   ... -> RelativeCoordinates -> RescaledObservation -> RepeatedRewardIndividualDone -> [AuxiliaryCameraRewards | AuxiliaryTargetRewards] -> FrameSkip(K)
 * hands the learner, as ONE launch (csrc/fragment_rows.hpp) over the rollout-shaped buffers of a K-frame launch: scalars [K][N][8], masks
 * [K][N][mask_words], the learner team's PLAIN observation rows [K][N][A][D].  live(f): the scalar record of frame f does not say done = 2.
 *   frames_dev  [N] int32: live frames; `last` is the greatest live f
 *   done_dev    [N] u8: 1 if a live frame says done = 1
 *   rewards_dev [N][4] f64: the frame-order sums over the live frames of the camera team reward, the target team reward, the normalised target team
 *               reward (scalar columns 0, 1, 7 widened to f64) and the negated third (the camera side's, environment.py:621-624)
 *   info_dev    [N][4] f64: the means over the live frames of coverage_rate and real_coverage_rate (frame-order sum / frames), mean_transport_rate and
 *               num_delivered_cargoes of frame `last` (FrameSkip.INFO_KEYS' 'mean' and 'last' entries; its 'sum' entries are rewards_dev)
 *   shaped_dev  [N][A] of `out_dtype`: the sum over the live frames of that frame's AuxiliaryCameraRewards / AuxiliaryTargetRewards row, exactly what
 *               `frames` accumulating launches of mate_engine_enable_reward_rows leave (same weighted sum, zero-coefficient skip, team `reduction`
 *               inside each frame).  `coefficients`: a HOST array [7] (camera) / [10] (target) in the order of mate_reward_rows, copied into an
 *               engine-owned device table the launch reads every time; mate_engine_fragment_coefficients returns that table, a schedule rewrites it
 *               in place between the replays of a captured graph.  Only the terms that are functions of the scalar record and the masks exist:
 *               soft_coverage_score, normalized_goal_distance, sparse_delivery and is_colliding need every frame's state, read NaN in the launch and a
 *               non-zero coefficient for one of them is refused (MATE_EINVAL, the message names the term).  num_tracked / is_tracked read that
 *               frame's camera -> target bits; the call must bring masks when one of them has a non-zero coefficient at enable (without masks they read 0).
 *   obs_dev     [N][A][D] of the engine's obs_dtype: frame `last`'s rows, through the optional column table (HOST arrays [D]; all four or none):
 *               out = ((v - own x) if column_sub = 1, (v - own y) if 2, v if 0; +0 where column_flag >= 0 and that column of the row reads 0)
 *               * column_scale + column_bias -- the operations and the order of the packer's fused transform (mate_engine_set_obs_transform) on the
 *               values the plain packer wrote: the rows equal the per-step flows' transformed rows bit for bit.
 * Any output may be NULL.  An environment without a live frame: frames 0, done 0, zero rewards / info / shaped; its observation row is not written.
 *
 * mate_engine_enable_fragment_rows (NULL `config` detaches): while attached, mate_engine_rollout_versus_greedy for `team` enqueues the launch BEHIND
 * the stepping launch (and the reward launch, if attached) and AHEAD of the restart of finished episodes, over the call's own buffers and its `steps`.
 * The call then needs io->scalars_dev 16-byte aligned and, where a mask term had a non-zero coefficient at enable, io->masks_dev (MATE_EINVAL).  No
 * allocation, no synchronisation, identical arguments at every call: capturable under mate_engine_device_tick.  Pipelined restarts return
 * MATE_ESTATE while attached.  No other call enqueues it.  A fused launch restarts finished episodes behind the launch WITHOUT packing their first
 * observation into caller buffers: a restarted environment hands the learner its terminal row, done set, for one fragment, as FrameSkip does before
 * the trainer's reset(), and its next action is chosen on that row -- unless mate_engine_enable_first_rows (below) is on.
 * mate_engine_fragment_rows: the on-demand form over any caller buffers (`rows`: camera_obs_dev or target_obs_dev of `team`, scalars_dev, masks_dev;
 * `frames` = K >= 1); uploads its tables (waits for the handle's launches).  frames = 1 over the per-step buffers gives the transformed reset() rows.
 * MATE_EINVAL: an unknown team, out_dtype or reduction, a camera team in a scenario without cameras, shaped rows without coefficients, a partial
 * column table, a refused term, misaligned buffers.  MATE_ESTATE: before the first reset / import_state. */
typedef struct mate_fragment_rows {
    int32_t team;                      /* MATE_TEAM_CAMERA / MATE_TEAM_TARGET: the learner's */
    void *obs_dev;
    double *rewards_dev, *info_dev;
    uint8_t *done_dev;
    int32_t *frames_dev;
    void *shaped_dev;
    int32_t out_dtype;                 /* of shaped_dev: MATE_OBS_F32 / MATE_OBS_F64 */
    int32_t reduction;                 /* MATE_REDUCE_* (MATE_REDUCE_MIN: the camera team's alone) */
    const double *coefficients;        /* host [7] / [10]; required with shaped_dev */
    const int32_t *column_sub, *column_flag;       /* host [D] */
    const double *column_scale, *column_bias;      /* host [D] */
} mate_fragment_rows;
int mate_engine_enable_fragment_rows(mate_engine *engine, const mate_fragment_rows *config);
int mate_engine_fragment_coefficients(mate_engine *engine, double **coefficients_dev, int32_t *count);
int mate_engine_fragment_rows(mate_engine *engine, const mate_fragment_rows *config, const mate_step_io *rows, int32_t frames, void *stream);

/* First rows of restarted episodes, for the attached fragment rows (opt-in; off, nothing above changes): the row every example trainer of the reference
 * gets from env.reset() once an episode has ended, and the per-step flows of this engine hand over in the call that restarts.  No kernel of its own and no
 * stepping kernel involved: the restart launch mate_engine_rollout_versus_greedy enqueues anyway (placement, occlusion tables, FIRST VIEW) already computes and
 * packs that row -- it now gets `rows_dev` as the attached team's observation pointer and `scalars_dev` as its scalar record -- and two more launches of the
 * fragment kernel with one frame move it into place.  While on, every mate_engine_rollout_versus_greedy for the attached team also enqueues
 *   behind the fragment launch: a memset node, every word of scalars_dev = 2.0f (no environment claims a restart this call did not make);
 *   its restart launch (immediate, or the interval's k-th under auto_reset = k > 1) with the two pointers: same episodes, records, masks and draws;
 *   behind that restart and ahead of the reward snapshot launch, only where the call enqueues the restart: obs_dev -> final_obs_dev (a plain copy; if set),
 *   then rows_dev -> obs_dev through the attached column table -- both only for the environments whose record the restart wrote.
 * After such a call, for an environment the call restarted (scalars_dev[env][2] != 2.0):
 *   obs_dev[env]        the new episode's first row through the fragment's transform: the per-step flows' row of the restarting call, bit for bit;
 *   final_obs_dev[env]  what obs_dev[env] would have shown without the feature: the terminal row, or, under a batched interval, the row it kept while
 *                       idling -- also where the environment ran no frame in this fragment (frames = 0: its obs_dev row, otherwise left unwritten, is replaced);
 *   done, frames, rewards, info, shaped: unchanged.  scalars_dev[env] is otherwise the restart's own record (done 0, the first view's coverage rates).
 * For every other environment obs_dev[env] is as without the feature and final_obs_dev[env] is untouched.  No allocation, no synchronisation, identical
 * arguments at every call: capturable under mate_engine_device_tick (the immediate restart is enqueued at every call, idle almost always, and so are the
 * two launches behind it).  A restart that closes an interval because the caller changed auto_reset or the flow (at the head of a LATER call, or in
 * mate_engine_device_tick) delivers no first rows: that call's own frames overwrite the rows.
 * A and D are the attached team's; the three buffers are caller-owned and distinct from obs_dev.  NULL `config` detaches; so does detaching the fragment rows,
 * or attaching them again for the other team or without obs_dev.
 * MATE_ESTATE: no fragment rows attached, or attached without obs_dev.  MATE_EINVAL: rows_dev or scalars_dev null or not 16-byte aligned, final_obs_dev not
 * aligned to its element, two of the buffers the same. */
typedef struct mate_first_rows {
    void  *rows_dev;       /* [N][A][D] obs_dtype: the learner team's PLAIN first rows (working buffer, caller-owned) */
    float *scalars_dev;    /* [N][8], 16-byte aligned: column 2 reads 2.0 unless the last attached call restarted the environment */
    void  *final_obs_dev;  /* [N][A][D] obs_dtype or NULL: the row obs_dev held before the first row replaced it */
} mate_first_rows;
int mate_engine_enable_first_rows(mate_engine *engine, const mate_first_rows *config);   /* NULL detaches */

/* FrameSkip fragments FRAME BY FRAME (csrc/frame_rows.hpp): the fragment above, built by one small launch behind each per-step call, so that a fragment of K
 * frames is K calls of mate_engine_step_versus_greedy -- against any opponent the per-step flows have (Heuristic, mixtures, channels) and with every shaping
 * term, since the per-step reward launch sees every frame's state.  The fused flow above stays exactly as it is; the two attach independently.
 * While attached, mate_engine_step_versus_greedy for `team` (no other call) enqueues fragment_frame_kernel behind the stepping launch, the reward launch and
 * the selection metrics and AHEAD of the restart (the fused fragment's position).  phase = the host's count of calls inside the open restart interval modulo
 * `frames`; live = the call's scalar record does not say done = 2.  Per environment:
 *   phase 0           frames_dev, done_dev, rewards_dev, info_dev, shaped_dev, restarted_dev are OVERWRITTEN with zeros first (no memset in front)
 *   a live frame      frames_dev += 1; done_dev |= (done == 1); rewards_dev += (f64) columns 0, 1, 7 and the negated 7, in frame order; info_dev[0..1] += columns
 *                     3, 4; info_dev[2..3] = columns 5, 6; shaped_dev[a] += the learner team's reward row of this call, in the row type
 *   phase frames - 1  info_dev[0..1] /= frames_dev (0 where it is 0)
 *   obs_dev           on the environment's last live frame of the fragment (done == 1, or live at the last phase) the learner team's rows of the call, a plain
 *                     copy: the packer's fused transform (mate_engine_set_obs_transform) has been applied.  No live frame: the row is not written.
 * With the Greedy opponents every tensor equals the fused fragment's bit for bit.  shaped_dev needs mate_engine_enable_reward_rows attached for `team` in
 * overwrite mode with the same out_dtype: its launch stays in overwrite mode, so the per-frame rows stay defined, and all of its terms are available.
 * first_rows != 0: on the call that closes a restart interval, behind the restart launch and ahead of the reward snapshot launch, the same kernel's second form
 * runs -- for every environment whose record of the call says done != 0 (what the restart has restarted): final_obs_dev <- obs_dev (if set), obs_dev <- the
 * call's rows (the restart has just packed the new episode's first rows there), restarted_dev = 1.
 * Every stepping call for `team` needs auto_reset = a positive multiple of `frames`, io->scalars_dev 16-byte aligned and the team's observation rows.  No
 * allocation, no synchronisation; under mate_engine_device_tick a captured interval has identical arguments at every replay.
 * mate_engine_frame_fragment: the on-demand form over caller buffers (`rows`: scalars_dev and the team's rows) -- closes = 0: the frame form at `phase`;
 * closes = 1: the second form (rows: the first rows), whatever first_rows says.  shaped_dev there reads the attached reward rows.
 * MATE_EINVAL: an unknown team or out_dtype, a camera team without cameras, frames < 1, phase outside [0, frames), a stepping call whose auto_reset is not a
 * positive multiple of frames or that lacks scalars_dev or the team's rows, info_dev without frames_dev, first_rows without obs_dev, buffers not aligned to their
 * element, obs_dev = final_obs_dev, shaped_dev with an out_dtype other than the attached reward
 * rows'.  MATE_ESTATE: shaped_dev while no overwrite-mode reward rows are attached for the team (at enable and at every call), attaching inside an open
 * restart interval, before the first reset, pipelined restarts while attached.  A refused call changes nothing.  NULL `config` detaches. */
typedef struct {
    int32_t team;                      /* MATE_TEAM_CAMERA / MATE_TEAM_TARGET: the learner's */
    int32_t frames;                    /* K >= 1 */
    void *obs_dev, *final_obs_dev;     /* [N][A][D] obs_dtype each, or NULL */
    uint8_t *restarted_dev;            /* [N] or NULL */
    double *rewards_dev, *info_dev;    /* [N][4] each, or NULL */
    uint8_t *done_dev;                 /* [N] or NULL */
    int32_t *frames_dev;               /* [N] or NULL */
    void *shaped_dev;                  /* [N][A] of out_dtype, or NULL */
    int32_t out_dtype;                 /* of shaped_dev: MATE_OBS_F32 / MATE_OBS_F64 */
    int32_t first_rows;                /* != 0: the second form behind the closing call's restart */
} mate_frame_fragments;
int mate_engine_enable_frame_fragments(mate_engine *engine, const mate_frame_fragments *config);
int mate_engine_frame_fragment(mate_engine *engine, const mate_frame_fragments *config, const mate_step_io *rows, int32_t phase, int32_t closes, void *stream);

/* Off-screen render: MultiAgentTracking.render(mode='rgb_array') (environment.py:986-1180) rasterised on the device (csrc/render_rows.hpp; the rules: DESIGN.md
 * section 3.20).  ONE launch on `stream` writes out_dev[count][size][size][3] uint8, frame k the picture of environment env_indices_dev[k] (any order, repeats
 * allowed; null: the environments 0 .. count - 1): the reference's display list point-sampled at the pixel centres of the view [-1050, 1050]^2, row 0 at the top,
 * white background, every primitive blended once per pixel in f32, one quantisation at the end.  The warehouse icons and the render callbacks are not drawn.
 * It reads the records and the engine's own mask words as the last call left them, and writes nothing but the frames.  The engine keeps that copy of the mask
 * words once mate_engine_keep_masks (that buffer alone) or mate_engine_policy_enable has allocated it: call either ahead of the reset; every launch that
 * writes a view fills it from then on, whether the call brings masks_dev or not.  headings_dev: [count][num_targets] f64, the reference's render-only target_orientations in degrees (the engine
 * keeps none); null: zeros.  No allocation, no synchronisation, identical arguments at every call: capturable.
 * MATE_EINVAL: count < 1, an index outside [0, N) (without indices: count > N; indices on the device are not read by the host -- the kernel leaves the frame
 * of an index outside [0, N) untouched), size outside [16, 4096], out_dev null or not 16-byte aligned, misaligned indices or headings, more tiles than one
 * launch takes.  MATE_ESTATE: before the first reset / import_state, or without the engine's own mask words; an argument error is reported
 * ahead of a state error.  A refused call changes nothing and launches nothing. */
#define MATE_RENDER_MIN_SIZE 16
#define MATE_RENDER_MAX_SIZE 4096
int mate_engine_keep_masks(mate_engine *engine);
int mate_engine_render(mate_engine *engine, const int32_t *env_indices_dev, int64_t count, int32_t size, const double *headings_dev, uint8_t *out_dev, void *stream);

/* Communication trace: the state of mate.RenderCommunication (mate/wrappers/render_communication.py) on the device (csrc/trace_rows.hpp; the rules: DESIGN.md
 * section 3.21).  Per enabled team an engine-owned uint8 matrix remaining[N][n sender][n recipient] and an int32 episode tag per environment.  While enabled,
 * every per-step call -- step, step_random, step_greedy, step_versus_greedy, step_selected, step_seated -- enqueues ONE more launch, comm_trace_kernel, behind
 * the agents' launches and ahead of the stepping launch (the wrapper updates before env.step).  For every environment that takes a live step in the call:
 * remaining = max(remaining - 1, 0), then remaining[s][r] = duration wherever a message s -> r was DELIVERED since the previous step -- the team's `delivered`
 * matrix of this call's agents' launch where it ran under a channel (mate_engine_set_channel: a team the engine plays WITHOUT a channel never materialises its
 * edges and marks nothing; a channel with default settings is transparent), the team's step_edges > 0 of mate_engine_route_messages since the last stepping
 * launch, both where both exist.  An environment idling under a batched restart keeps its bytes.  A launch that finds an episode number other than the tag starts
 * that environment from zeros and retags it (the wrapper's reset()): resets and restarts need no launch; enable, mate_engine_seed and mate_engine_import_state
 * clear the tags.  mate_engine_render draws the arrows of every enabled team's matrix whose tag is the environment's episode number, at the wrapper's list
 * position: behind the obstacles, ahead of the first camera's sector.
 * mate_engine_enable_comm_trace: teams_mask = 1 << MATE_TEAM_CAMERA, 1 << MATE_TEAM_TARGET or both (0 detaches; the buffers stay the engine's), duration in
 * [1, 255] (the wrapper's default: 20); the enabled matrices start from zeros.  MATE_EINVAL: a mask outside [0, 3], a duration outside [1, 255], a team
 * without agents.  Under a mixture the `delivered` rows of the environments whose episode drew a candidate that does not talk read zero, and a team of Naive / Random
 * agents alone is not in the agents' launch: nothing is marked.  While enabled, mate_engine_rollout_random, _rollout_greedy and _rollout_versus_greedy (their frames'
 * edges are never materialised: step per frame) and every call with auto_reset = MATE_RESET_PIPELINED return MATE_ESTATE.  A refused call changes nothing.
 * mate_engine_comm_trace: the engine-owned matrix and tags of an enabled team (either pointer may be null).
 * mate_engine_set_comm_trace: copies the caller's [N][n][n] matrix on the device into the engine's and tags every environment with its current episode number;
 * complete when the call returns.  MATE_ESTATE: the team is not enabled, or before the first reset / import_state. */
int mate_engine_enable_comm_trace(mate_engine *engine, int32_t teams_mask, int32_t duration);
int mate_engine_comm_trace(mate_engine *engine, int32_t team, uint8_t **remaining_dev, int32_t **tag_dev);
int mate_engine_set_comm_trace(mate_engine *engine, int32_t team, const uint8_t *remaining_dev);

/* Per-episode metric records (csrc/episode_rows.hpp): what the reference's example trainers report at every episode's end (examples/utils/callbacks.py:
 * MetricCollector's mean over the agents of each learner step's infos, CustomMetricCallback.on_episode_end's mean / last / episode_<key> sums over the
 * episode's steps), kept on the device for ONE team's perspective.  While attached every stepping call -- step, step_random, step_greedy,
 * step_versus_greedy, step_selected, rollout_random, rollout_greedy, rollout_versus_greedy -- enqueues one more launch, episode_rows_kernel, behind the
 * reward and the fragment launch and ahead of the restart; no stepping kernel is involved.  A learner step is one frame of the call whose scalar record does
 * not say done = 2 -- also in a mate_engine_rollout_versus_greedy call with fragment rows attached: a fragment counts as its frames, not as one step.  The
 * running sums live in an engine-owned table across launches; a learner step that says done = 1 appends ONE record of MATE_EPISODE_COLUMNS doubles and
 * clears them:
 *    0 env (first_env_index + i)   1 episode (the engine's episode number, the one in the Philox key)   2 steps (learner steps)   3 frames (live frames)
 *    4 length (the engine's episode step count at the end: frames == length says the record covers the whole episode)
 *    5 episode_raw_reward (the team's reward)   6 episode_normalized_raw_reward   7 episode_reward (the agent-order sum of the learner's reward row: the
 *      attached reward rows of the team in a one-frame call in overwrite mode, else the team reward once per agent; NaN where shaped rows exist but do
 *      not describe every step: accumulate mode, a multi-frame call, a fragment's shaped rows)
 *    8 raw_reward = [5] / steps   9 normalized_raw_reward = [6] / steps   10 coverage_rate   11 real_coverage_rate (step-order sums / steps)
 *   12 mean_transport_rate   13 num_delivered_cargoes (of the last step)
 *   14 num_tracked: cameras, and only where every call brought io->masks_dev (NaN otherwise): popcount of the camera -> target bits / cameras per frame,
 *      step-order sum / steps
 *   15 team
 * Every sum is f64 in step order, product then add.  Record number n (counted from 0 in *count_dev, which the caller zeroes and the engine only adds to)
 * lives in slot n % capacity of records_dev [capacity][MATE_EPISODE_COLUMNS]; older records are overwritten; the order among the environments that
 * finish in one launch is unspecified.  capacity >= num_envs keeps the launch parallel (one atomic add per wave); a smaller ring is served by one
 * serial workgroup.  A reset of an environment (reset, masked reset, reset_tape, a restart, import_state) discards its sums without a record, and
 * so does seed(); after import_state the episodes in progress give records with frames < length.  The calls then need io->scalars_dev, 16-byte
 * aligned (MATE_EINVAL); pipelined restarts return MATE_ESTATE.  No allocation, no synchronisation, identical arguments at every call: capturable.
 * records_dev == NULL detaches.
 * MATE_EINVAL: an unknown team, a camera team in a scenario without cameras, capacity < 1, a null counter, buffers not 8-byte aligned.
 * MATE_ESTATE: before the first reset / import_state.
 * mate_engine_clear_episode_records forgets the episodes in progress (an async memset on `stream`); the ring and the counter are the caller's. */
#define MATE_EPISODE_COLUMNS 16
int mate_engine_enable_episode_records(mate_engine *engine, int32_t team, double *records_dev, int64_t capacity, int64_t *count_dev);
int mate_engine_clear_episode_records(mate_engine *engine, void *stream);

/* MoreTrainingInformation rows (csrc/info_rows.hpp): what the reference's mate.MoreTrainingInformation wrapper
 * (wrappers/more_training_information.py:42-98) adds to every agent's info at a step, as three f64 outputs per environment (integers and booleans stored
 * exactly as doubles; the column order is the ABI):
 *   camera_rows_dev [N][Nc][MATE_INFO_CAMERA_COLUMNS]   0 num_tracked = camera_target_view_mask[c, :].sum()   1 is_sensed = target_camera_view_mask[:, c].any()
 *   target_rows_dev [N][Nt][MATE_INFO_TARGET_COLUMNS]   0 goal (-1: none)   1 goal_distance (warehouse_distances[goal]; 1000 without a goal)
 *       2 .. 5 warehouse_distances = max(|location - WAREHOUSES[w]| - 75, 0)   6 individual_done (target_dones[t]: the goal differs from the goal before this
 *       step and that goal was >= 0)   7 is_tracked = camera_target_view_mask[:, t].any()   8 is_colliding
 *   cargo_rows_dev  [N][MATE_INFO_CARGO_COLUMNS]        0 .. 3 remaining_cargo_counts   4 .. 7 awaiting_cargo_counts   8 .. 23 remaining_cargoes [warehouse][destination]
 * The wrapper's other keys exist already: `state` is the state rows; the five masks are the call's mask words; camera_states / target_states are the private
 * slices of the plain observation rows; obstacle_states is part of the state row.
 * mate_engine_enable_info_rows attaches one launch, info_rows_kernel, behind every stepping call -- step, step_random, step_greedy, step_versus_greedy,
 * step_selected, rollout_random, rollout_greedy, rollout_versus_greedy -- behind the reward launch and ahead of the restart: the rows describe the step the
 * call's scalar record describes, the terminal one included.  A multi-frame call leaves the rows of its LAST frame, with individual_done = NaN (a delivery
 * between the frames cannot be seen from the end state); the goals of that frame are what the next call compares with.  individual_done is measured against an
 * engine-owned snapshot of the previous step's goals and episode number, independent of the reward rows': a step of another episode than the snapshot's
 * reports 0; every reset, masked reset, reset_tape, restart and import_state is followed by a snapshot-only launch.  An environment whose record says done = 2
 * keeps its rows and its snapshot untouched; a reset does not rewrite the rows (the reference has no info at reset()); observe() does not run the launch.
 * The buffers are the caller's, 16-byte aligned; a null pointer means that output is not written; all three null detaches.  While attached the calls need
 * io->scalars_dev and io->masks_dev (MATE_EINVAL); pipelined restarts return MATE_ESTATE.  No allocation, no synchronisation, identical arguments at every
 * call: capturable.
 * MATE_EINVAL: a misaligned buffer, camera rows in a scenario without cameras.  MATE_ESTATE: before the first reset / import_state.
 * mate_engine_info_rows is the same launch on demand, from the current records, nothing attached: individual_done reads NaN and no snapshot is touched;
 * masks_dev ([N][mask_words], e.g. the last call's) may be null: num_tracked, is_sensed and is_tracked then read NaN. */
#define MATE_INFO_CAMERA_COLUMNS 2
#define MATE_INFO_TARGET_COLUMNS 9
#define MATE_INFO_CARGO_COLUMNS 24
int mate_engine_enable_info_rows(mate_engine *engine, double *camera_rows_dev, double *target_rows_dev, double *cargo_rows_dev);
int mate_engine_info_rows(mate_engine *engine, const uint32_t *masks_dev, double *camera_rows_dev, double *target_rows_dev, double *cargo_rows_dev, void *stream);

/* Occlusion table of one camera (Camera.sight_range_func, entities.py:457-479): host buffers. */
int mate_engine_lut_read(mate_engine *engine, int64_t env, int32_t camera, double *phis_host,
                         double *rhos_host, int32_t capacity, int32_t *count);

/* The outer occlusion boundary, Camera.boundary_outer / sight_range_outer_func (entities.py:419-448, 479), read by
 * boundary_between(outer=True) (entities.py:513-543: AuxiliaryCameraRewards' soft coverage score and the renderer).
 * Off by default; once enabled every reset / rebuild_luts builds it next to the inner table (`*capacity` = knots
 * per camera to provide to lut_read_outer).  360 + 223 * obstacles rays per table: sorted in the LDS up to 16 obstacles, in HBM scratch beyond. */
int mate_engine_enable_outer_boundary(mate_engine *engine, int32_t *capacity);
int mate_engine_lut_read_outer(mate_engine *engine, int64_t env, int32_t camera, double *phis, double *rhos,
                               int32_t capacity, int32_t *count);
/* Install a recorded outer table (what sight_range_outer_func.x / .y hold, closing knot included). */
int mate_engine_lut_write_outer(mate_engine *engine, int64_t env, int32_t camera, const double *phis_host,
                                const double *rhos_host, int32_t count);
/* AuxiliaryCameraRewards' soft coverage score of the current state (wrappers/auxiliary_camera_rewards.py:181-239
 * compute_soft_coverage_scores, :128-139 per-camera reduction): `matrix_dev` [N][Nc][Nt] f64 (or NULL) receives
 * +-distance(target, nearest point of the camera's sector outline) / radius of the sector's inscribed circle, signed by
 * camera_target_view_mask; `scores_dev` [N][Nc] f64 (or NULL) the sum over the targets a camera tracks, or tanh(max)
 * when it tracks none.  `masks_dev` = the packed masks of the step / reset this follows ([N][mask_words] uint32, as
 * mate_step_io.masks_dev).  Needs the outer boundary (enable + a reset or rebuild_luts since); environments whose outer
 * table was never built yield NaN. */
int mate_engine_soft_coverage(mate_engine *engine, const uint32_t *masks_dev, double *matrix_dev, double *scores_dev, void *stream);
int mate_engine_lut_write(mate_engine *engine, int64_t env, int32_t camera, const double *phis_host,
                          const double *rhos_host, int32_t count);
/* Rebuild the occlusion tables of all environments from the current static geometry
 * (Camera.add_obstacles, entities.py:362-479) -- used after mate_engine_import_state. */
int mate_engine_rebuild_luts(mate_engine *engine, void *stream);

/* Number of (environment, step) slots spent idle waiting for a batched reset (auto_reset > 1) since creation:
 * executed env-steps = N * calls - idle. */
int mate_engine_idle_steps(mate_engine *engine, int64_t *total);

/* Average duration (ms) of the dominant kernel (step_kernel) over the launches timed since the
 * previous call, measured with HIP event pairs on the launch stream (bench.py roofline).
 * `enable` = k > 0 arms the timer for every k-th step launch from now on, 0 disarms it. */
int mate_engine_kernel_time(mate_engine *engine, int32_t enable, double *avg_ms, int64_t *launches);

/* Which compilation of the step kernel the last step()/step_random() launch ran: 0 = the generic flow (every launch
 * switch read on the device), 1 = the on-device random policy flow, 2 = the f32-continuous-actions flow.  1 and 2 are
 * the same code with the switches folded at compile time (no tapes, no discrete actions, plain observations, all four
 * outputs present, immediate auto-reset); results are bit-identical.  MATE_FLOW_GENERIC=1 forces 0.
 * After a launch with the on-device agents: 3 = rollout_greedy_kernel (the fused rollouts; a per-step call under
 * MATE_STEP_GREEDY_ROLLOUT=1), 4 = step_greedy_kernel (the one-launch form of step_greedy / step_versus_greedy). */
int mate_engine_last_flow(const mate_engine *engine);

/* Device memory for the [steps][N][...] observation blocks of the fused rollouts (mate_step_io.camera_obs_dev /
 * target_obs_dev of mate_engine_rollout_*), laid out for the way those kernels write: every environment-wave streams its
 * own 2-4 KB rows, thousands of rows at a time, and how fast HBM takes that depends on where the pages lie -- blocks from
 * hipMalloc measured 4.3-5.6 TB/s from one allocation to the next on the same GPU, physically contiguous ones
 * (hipDeviceMallocContiguous) 2.9-3.2 TB/s, the same block built from 2 MiB physical chunks mapped in a SHUFFLED order
 * 5.4-5.8 TB/s (tools/store_vmm.hip).  block_alloc builds such a block (hipMemCreate / hipMemMap, the virtual range is
 * contiguous); any device pointer works in mate_step_io -- this one is only faster to write.  `bytes` is rounded up to
 * 2 MiB.  block_free unmaps the block chunk by chunk (one hipMemUnmap per hipMemMap) and releases its memory; the virtual
 * range stays reserved (address space only; MATE_BLOCK_FREE_RANGE above).  The pointer must come from block_alloc; the CALLER
 * has waited for every launch that reads or writes the block -- the library does not synchronise here.  A failed block_alloc / block_probe / block_free reports through its return code
 * only: HIP's sticky last-error is cleared, so the caller's next launch check does not see it. */
/* The form of the row stores of the row-image rollouts (MATE-4v8-9, MATE-4v8-0, MATE-4v2-9, MATE-Navigation under mate_engine_rollout_random): 0 (default) the
 * rows' 16-byte chunks as they lie -- 1.3-2 % faster where the blocks take the rows fast, i.e. where the arithmetic bounds a launch
 * --, 1 every store instruction an aligned kilobyte -- 3 % faster where they do not (mate_engine_block_probe of the target block
 * below ~4.8 TB/s: the stores bound the launch).  Same rows either way.  Engine.reserve_rollout sets it from what it probed. */
int mate_engine_set_store_form(mate_engine *engine, int32_t shifted);
int mate_engine_block_alloc(int32_t device, int64_t bytes, void **ptr_out);
int mate_engine_block_free(void *ptr);
/* How fast THIS block takes the fused rollouts' stores: a store-only launch with their shape (one wave per environment, four
 * per workgroup, `rows_per_step` environments, `row_bytes` per environment and step -- a multiple of 16 --, a kilobyte of
 * non-temporal 16-byte stores per instruction) over the whole block, best of three, in GB/s.  Shuffled chunks
 * make a slow block unlikely, not impossible (one in four on some GPUs of the pool): a caller that has memory to spare allocates
 * a few candidates, keeps the fastest and frees the rest -- Engine.reserve_rollout does.  The block is left filled with zeros. */
int mate_engine_block_probe(int32_t device, void *block, int64_t bytes, int32_t rows_per_step, int32_t row_bytes, void *stream,
                            double *gbytes_per_s);
/* Environments per wave of the fused rollouts (mate_engine_rollout_random / _rollout_greedy / _rollout_versus_greedy) and of mate_engine_step /
 * _step_random / _step_greedy / _step_versus_greedy (which run the same kernels with one step where the choice below says so).  The engine maps ONE
 * environment onto one 64-lane wave; the small scenarios (at most four cameras and four targets: MATE-{1v1,1v2,2v2,2v4,4v2,4v4}-{0,9}, e.g. the
 * MATE-2v4-0 of the reference's target trainers, examples/ippo/target/config.py:63-66) fill a quarter of one, so their fused rollouts
 * can step FOUR environments per wave, sixteen lanes each -- same results, bit for bit.  `enable`: 0 = one per wave; 1 = the shape's
 * own number in every fused launch; 2 (the default; MATE_SUBWAVE=0 / MATE_SUBWAVE=1 in the environment make 0 / 1 the default) = where it measured faster:
 * batches of at least 32 environments per compute unit, and under the random policy every such shape but MATE-4v4-* (whose
 * one-per-wave rollout, carried by the register-resident row image, is as fast); negative = leave it as it is.  `*in_use` (may be NULL) receives
 * the number ONE flow now runs with: the fused Greedy rollouts (mate_engine_rollout_greedy / _rollout_versus_greedy), exactly as their launch is
 * planned, the fit of the sub-wave workgroup in the LDS included (1 for a shape without such kernels).  The other flows decide on top of it: the
 * random-policy flows and mate_engine_step / _step_random keep one per wave for MATE-4v4-* in mode 2 and for MATE-4v8-0 always, the per-step
 * flows follow MATE_STEP_SUBWAVE, f64 observations always run one per wave.  Takes effect from the next launch on; no state changes. */
int mate_engine_set_sub_wave(mate_engine *engine, int32_t enable, int32_t *in_use);
/* The HBM rates of THIS GPU as this library's own streaming kernels see them (the yardsticks beside the vendor peak in bench.py's
 * roofline object): `mode` 0 = read `src` and write `dst` (read + write bytes counted), 1 = write `dst` only (non-temporal stores, as the row
 * writers), 2 = read `src` only, 3 = write `dst` only with plain stores (a memset);
 * 16 bytes per lane, grid-stride over `bytes` (use >= 1 GiB), non-temporal, median of five launches timed with HIP events on `stream`.
 * No reference counterpart: measurement support (SURVEY.md section 8d "confirm on the box"). */
int mate_engine_hbm_probe(int32_t device, const void *src, void *dst, int64_t bytes, int32_t mode, void *stream, double *gbytes_per_s);
/* Physical device memory taken and held without being mapped (hipMemCreate in 256 MiB pieces), and given back: what a search
 * for a fast block puts between two candidates so that the next one comes from further into the device's memory -- the blocks'
 * chunks come out of the same pool, in order; memory from hipMalloc does not move that pool's cursor. */
int mate_engine_memory_hold(int32_t device, int64_t bytes, void **token_out);
int mate_engine_memory_release(void *token);

/* Communication channels for the scripted agents' messages: the reference's NoCommunication, RandomMessageDropout, RestrictedCommunicationRange
 * and MessageFilter wrappers (mate/wrappers/) on the device.  A channel belongs to a TEAM (MATE_TEAM_CAMERA / MATE_TEAM_TARGET) and decides, per step
 * and per routed message sender -> recipient of that team's Greedy agents (and of the Heuristic targets, which inherit the Greedy targets' exchange),
 * whether the message arrives: only where the team is not `disabled`, norm2(recipient - sender) <= `range_limit` (< 0 or +inf: no limit), the
 * pair's binomial(1, dropout_rate) draws 0 (u > 1 - p for p <= 0.5, else u <= p, draws 1), and the pair's byte of `mask_dev` ([N][n][n] uint8,
 * [sender][recipient], read at every launch; NULL: all ones) is non-zero.  The sender never knows: a Greedy camera redraws its delay and clears its
 * message, a broadcasting target clears its flag; only delivered messages change the recipients' memory.  Naive and Random agents send nothing.
 *
 * mate_engine_set_channel needs mate_engine_policy_enable (MATE_ESTATE otherwise), waits for the handle's launches, and may change at any call
 * boundary; NULL clears the team's channel.  MATE_EINVAL: a team that is neither, a rate outside [0, 1] or not finite, a NaN range_limit.  MATE_ESTATE:
 * a camera channel while the Heuristic camera agent is selected or is a mixture candidate with positive weight (its fallback when a response is lost is an
 * assignment solve the device does not have) -- and selecting or installing that opponent while a camera channel is set.  A refused call changes nothing.
 * While a channel is set for a team whose communicating agents act in a call, mate_engine_step_greedy / _step_versus_greedy / _step_selected take the
 * two-launch form with greedy_channel_kernel as the agents' launch (capturable under mate_engine_device_tick: identical arguments, no allocation, no
 * synchronisation), and mate_engine_rollout_greedy / _rollout_versus_greedy return MATE_ESTATE: step per frame.  A channel of the caller's own team, or of
 * a team nobody of the Greedy / Heuristic-target agents plays in the call, is inert: same flow, same bytes.
 * Not provided: ExtraCommunicationDelays (a queue of stale message contents per pair; not used by the reference's evaluation script).
 *
 * mate_engine_channel_tape: the dropout uniforms of the two teams, [N][n][n] f64 [sender][recipient] (NULL: Philox, stream 26, keyed by seed, global
 * environment index, tick and team << 8 | sender << 4 | recipient), and buffers that receive the uniform every verdict used (NaN where none was drawn;
 * NULL: not stored).  All four hold until replaced.
 * mate_engine_channel_edges: the team's two engine-owned int8 matrices [N][n][n], as the last agents' launch with a channel left them: `sent` (what the agents
 * handed to the channel) and `delivered` (what arrived: the reference's camera_ / target_communication_edges).  An environment that launch skipped keeps its rows. */
typedef struct { int32_t disabled; double range_limit; /* < 0 or +inf: none */ double dropout_rate; const uint8_t *mask_dev; } mate_channel;
int mate_engine_set_channel(mate_engine *engine, int32_t team, const mate_channel *cfg);      /* NULL clears */
int mate_engine_channel_tape(mate_engine *engine, const double *camera_u_dev, const double *target_u_dev,
                             double *record_camera_u_dev, double *record_target_u_dev); /* [N][n][n]; NULL: Philox / not stored */
int mate_engine_channel_edges(mate_engine *engine, int32_t team, int8_t **sent_dev, int8_t **delivered_dev);

/* A learner seat among on-device teammates: the reference's SingleCamera / SingleTarget wrappers (mate/wrappers/single_team.py, SingleTeamSingleAgent) on the
 * device.  The learner plays ONE slot of `team`, the seat; the team's other n - 1 slots are its Greedy agents with their true indices, the opposing team is
 * whatever mate_engine_set_*_opponent / _set_opponent_mixture make of it.  Around the seat the teammates behave as the reference's: a Greedy camera teammate
 * sends its one 'state' message to the seat (and draws that pair's delay) and never again, since the seat never answers and never becomes a neighbour; Greedy target
 * teammates broadcast to every slot; the seat itself sends nothing, draws nothing and keeps no memory.  The learner's own messages are not provided.
 *
 * The seat of an episode is a pure function: MATE_SEAT_FIXED a constant (`fixed_seat`, < 0: n - 1, the wrapper's index with shuffle_entities off);
 * MATE_SEAT_DRAW (uint64(philox(seed, global environment index, episode, stream 27, team).x) * n) >> 32, drawn anew for every episode (shuffle_entities on);
 * MATE_SEAT_TAPE the caller-owned `seat_tape_dev` ([N] int32, read at every launch; a value outside [0, n) falls back to MATE_SEAT_DRAW).
 *
 * mate_engine_enable_seat: the caller's buffers `obs_out_dev` ([N][D_team] obs_dtype, 16-byte aligned: the seat's row of the call's output observations),
 * `seat_index_dev` ([N] int32: the seat of the episode that row belongs to -- after an immediate restart the NEW episode's) and `seat_acted_dev` ([N] int32: the
 * seat whose action the last mate_engine_step_seated consumed).  All three NULL: disable.  One seat team per engine.  Enabling, changing or disabling the seat marks
 * that team's Greedy agents for their reset at their next acting call.  It needs mate_engine_policy_enable (MATE_ESTATE otherwise) and waits for the handle's launches.
 * MATE_EINVAL: a team that is neither, a team without agents, a fixed seat outside [0, n), MATE_SEAT_TAPE without a tape, a missing or misaligned buffer.
 * MATE_ESTATE: a seat on a team with a Heuristic selection, a mixture other than {Greedy} or a channel set -- and installing any of these on the seat team while
 * the seat is enabled; a seat while the opposing team's channel is live (that flow's agents' launch is greedy_channel_kernel).  A refused call changes nothing.
 *
 * mate_engine_step_seated: `io`'s action pointer of the seat team holds the seat's action, [N][2] f32 / f64 pairs or [N] int32 grid indices with that team's
 * *_DISCRETE bit; the other team's action pointer is ignored.  `tape` keeps its full shapes; the seat's entries are ignored.  Launches: greedy_seat_kernel (both
 * teams' agents, the seat's lane writing the learner's action into the team's joint row), whatever the opposing team's plan adds (Heuristic cameras, drift, scripted
 * launch), the stepping launch on both teams' engine-owned rows (mate_engine_policy_actions returns them), the attached launches and the restart as for
 * mate_engine_step_greedy, seat_rows_kernel last.  Identical arguments at every call, no allocation, no synchronisation: capturable under
 * mate_engine_device_tick.  An environment idling under a batched restart keeps its row, its seat_index and its seat_acted.  Reward and done are team-level:
 * the scalar rows.  mate_engine_rollout_greedy / _rollout_versus_greedy and the fragment rows are untouched: there is no fused K-frame seat flow (FrameSkip is K
 * calls with the action held).  With a seat enabled and mate_engine_step_seated never called, every other entry point gives the bytes it gives without.
 * mate_engine_seat_rows: the gather on demand (behind a reset): every environment's row and seat from `io`'s observation rows of the seat team. */
#define MATE_SEAT_FIXED 0
#define MATE_SEAT_DRAW 1
#define MATE_SEAT_TAPE 2
int mate_engine_enable_seat(mate_engine *engine, int32_t team, int32_t mode, int32_t fixed_seat, const int32_t *seat_tape_dev,
                            void *obs_out_dev, int32_t *seat_index_dev, int32_t *seat_acted_dev);      /* the three outputs NULL: disable */
int mate_engine_step_seated(mate_engine *engine, const mate_step_io *io, const mate_policy_tape *tape, int32_t auto_reset, void *stream);
int mate_engine_seat_rows(mate_engine *engine, const mate_step_io *io, void *stream);

/* The learner's own messages through the team's channel: the environment's send_messages / receive_messages and the communication-edge counts of `info`
 * (mate/environment.py) under the channel wrappers, as one launch on demand (csrc/message_rows.hpp: message_rows_kernel).  A message is `width` numbers of
 * obs_dtype from sender s to recipient r of one team; one routing call handles at most one message per ordered pair and team.  `payload_dev` is [N][n][width]
 * (one content per sender, to everyone it addresses) or, `pairwise`, [N][n][n][width] ([sender][recipient]).  `address_dev`: [N][n][n] uint8, [sender][recipient],
 * non-zero = addressed, read at every launch; NULL: broadcast, to every slot of the team, the sender's own included (an edge like any other, distance 0).  A sent
 * message arrives iff the team's channel (mate_engine_set_channel: disabled, range_limit over the positions of the current records, dropout_rate, mask) lets it;
 * with no channel set everything arrives.  `inbox_dev`: [N][n recipient][n sender][width], the delivered content, zeros where nothing was sent or nothing arrived;
 * the launch writes the whole block.  payload_dev and inbox_dev must be 16-byte aligned.
 *
 * mate_engine_enable_messages: per team; a NULL cfg disables.  It waits for the handle's launches and needs no mate_engine_policy_enable: the router reads the
 * environments' records and the channel's settings, nothing of the on-device agents (mate_engine_set_channel itself needs it).  MATE_EINVAL: a team that is
 * neither, a team without agents, a width outside [1, 65536], a missing or misaligned buffer.  A refused call changes nothing.  Enabling starts the counts afresh.
 * mate_engine_route_messages: `team_mask` is 1 << MATE_TEAM_CAMERA, 1 << MATE_TEAM_TARGET or both, `round` lies in 0..15 and enters the draws' key (the
 * reference's agents talk twice per step; a learner may route several times between two steps).  One launch for both teams; identical arguments at every call, no
 * allocation, no synchronisation: capturable under mate_engine_device_tick.  MATE_EINVAL: a mask outside 1..3, a round outside 0..15.  MATE_ESTATE: a team of
 * the mask that is not enabled, or no reset so far.  An environment whose episode is over (finished, waiting for a batched restart or for the caller's reset) is
 * skipped and keeps every row.  Routing a team whose Greedy agents also act is allowed and does not reach them: their exchange is reference-format and stays
 * where it is; no stepping flow changes a byte with messages enabled.
 * Draws: one uniform per (team, round, sender, recipient), only where the team's dropout rate is > 0 and the message was sent: mate_engine_message_tape's
 * [N][n][n] f64 tapes (NULL: Philox, stream 28, keyed by seed, global environment index, tick and round << 12 | team << 8 | sender << 4 | recipient, word .x as
 * a 32-bit uniform -- independent of first_env_index and of sharding); its record buffers receive the uniform each verdict used, NaN where none was drawn.  All
 * four hold until replaced.
 * mate_engine_message_edges: the team's engine-owned matrices -- `sent`, `delivered` (int8 [N][n][n], [sender][recipient], of the last routing call), `step_edges`
 * (int32 [N][n][n]: the deliveries since the last stepping launch, the reference's camera_ / target_communication_edges, which step reports and clears; two
 * rounds of a pair within one step count 2), `total_edges` (int32 [N][n][n]: the reference's *_total_communication_edges of the episode as its last step left
 * them, i.e. without the current step's), `agent_edges` (int32 [N][n][2]: out_ and in_communication_edges of `info`, the row and column sums of step_edges).  A
 * (tick, episode) tag per team and environment in engine memory makes the counts a function of what a routing launch sees: a tick other than the tag's folds
 * step_edges into total_edges and zeroes it, an episode other than the tag's zeroes both; mate_engine_seed, a reset of the whole batch and
 * mate_engine_import_state clear the tags.  MATE_ESTATE before the team's first mate_engine_enable_messages. */
typedef struct { int32_t width, pairwise; const void *payload_dev; const uint8_t *address_dev; void *inbox_dev; } mate_message_rows;
int mate_engine_enable_messages(mate_engine *engine, int32_t team, const mate_message_rows *cfg);      /* NULL disables */
int mate_engine_route_messages(mate_engine *engine, int32_t team_mask, int32_t round, void *stream);
int mate_engine_message_edges(mate_engine *engine, int32_t team, int8_t **sent_dev, int8_t **delivered_dev, int32_t **step_edges_dev, int32_t **total_edges_dev,
                              int32_t **agent_edges_dev);
int mate_engine_message_tape(mate_engine *engine, const double *camera_u_dev, const double *target_u_dev, double *record_camera_u_dev, double *record_target_u_dev);

#ifdef __cplusplus
}
#endif
#endif /* MATE_ENGINE_H */
