// instrument.hpp -- the profiling hooks of the step, rollout and Greedy kernels, all in one place.  The shipped library defines
// neither switch below, and every hook is then empty:
//
//   -DMATE_PHASE_CLOCKS  the profiling build (python -m mate_amd.build --prof: lib/libmate_engine_prof.so, selected with
//                        MATE_ENGINE_LIB by tools/*_phases.py): s_memtime stamps, one row of kClockStride slots per environment
//                        in Ptrs::phase_clocks (mate_engine_debug_phase_clocks), and Ptrs::debug_skip (SKIP) drops phases of
//                        step_kernel (tools/phase_profile.py)
//   -DMATE_ISA_MARKS     phase boundaries as comments in the -S output, no instruction emitted (tools/isa_phases.py reads the
//                        MATE_PHASE_END marks of rollout_kernel)
//
// The slots of a row, per kernel:
//   step_kernel            0 begin, 1-8 phase boundaries (PHASE_STAMP), 9-14 inside the kinematics and the view (SUB_STAMP),
//                          15 the wave's lifetime in 100 MHz ticks
//   step_split_kernel      0-7 wave A (cameras), 8-15 wave B (targets) (SPLIT_STAMP)
//   rollout_kernel         0-7 cycles per phase summed over the launch's steps (ROLL_STAMP), 8-11 the prologue and 12 the epilogue
//                          in cycles since the wave began (PROLOGUE_STAMP), 13 HW_ID | XCC_ID << 32, 14 / 15 the step loop in
//                          s_memtime / 100 MHz ticks
//   rollout_greedy_kernel  0-6 as in rollout_kernel, 7 the loop head, 8 agents observe, 9 the zoom solve, 10 the actions,
//                          11 communicate, 12 choose (GREEDY_STAMP, POL_STAMP), 14 / 15 as in rollout_kernel
//   step_greedy_kernel     0-8 phase boundaries (SG_STAMP), 9-13 the agents' sub-phases 8-12 of greedy_policy_body (POL_STAMP),
//                          15 the wave's lifetime in 100 MHz ticks
// The stamps read the kernel's own `lane`, `g` and `env` (SPLIT_STAMP also `role`), the accumulating ones `acc` and `t_prev`,
// PROLOGUE_STAMP `t_wave`: what a kernel declares for them is wrapped in MATE_PROF, which only the profiling build compiles.
#pragma once

namespace mate {
constexpr int kClockStride = 16;      // stamps per environment in Ptrs::phase_clocks
}

#if defined(MATE_PHASE_CLOCKS)
#define MATE_PROF(...) __VA_ARGS__
#define SKIP(bit) (g.debug_skip & (bit))
#define PHASE_STAMP(i) do { if (lane == 0 && g.phase_clocks) g.phase_clocks[env * kClockStride + (i)] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
#define SUB_STAMP(c, i) do { if ((c).lane == 0 && (c).g.phase_clocks) (c).g.phase_clocks[(c).env * kClockStride + (i)] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
#define SG_STAMP(i) PHASE_STAMP(i)
#define SPLIT_STAMP(i) do { if (lane == 0 && g.phase_clocks) g.phase_clocks[env * kClockStride + role * 8 + (i)] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
#define PROLOGUE_STAMP(i) do { if (lane == 0 && g.phase_clocks) g.phase_clocks[env * kClockStride + (i)] = (long long)__builtin_amdgcn_s_memtime() - t_wave; } while (0)
#define ROLL_STAMP(i) do { const long long t_now = (long long)__builtin_amdgcn_s_memtime(); acc[i] += t_now - t_prev; t_prev = t_now; } while (0)
#define GREEDY_STAMP(i) ROLL_STAMP(i)
// greedy_policy_body: into the caller's accumulators, passed as PROF_ACC(acc, t_prev)
#define POL_STAMP(i) do { if (acc) { const long long t_now = (long long)__builtin_amdgcn_s_memtime(); acc[i] += t_now - *t_prev; *t_prev = t_now; } } while (0)
#define PROF_ACC(acc, t_prev) acc, &t_prev
#elif defined(MATE_ISA_MARKS)
#define MATE_PROF(...)
#define SKIP(bit) false
#define PHASE_STAMP(i) asm volatile("; ==== MATE_STEP_PHASE " #i)
#define SUB_STAMP(c, i) asm volatile("; ==== MATE_STEP_SUB " #i)
#define SG_STAMP(i) do { } while (0)
#define SPLIT_STAMP(i) do { } while (0)
#define PROLOGUE_STAMP(i) do { } while (0)
#define ROLL_STAMP(i) asm volatile("; ==== MATE_PHASE_END " #i)
#define GREEDY_STAMP(i) asm volatile("; ==== MATE_GREEDY_PHASE " #i)
#define POL_STAMP(i) asm volatile("; ==== MATE_GREEDY_PHASE " #i)
#define PROF_ACC(acc, t_prev) nullptr, nullptr
#else
#define MATE_PROF(...)
#define SKIP(bit) false
#define PHASE_STAMP(i) do { } while (0)
#define SUB_STAMP(c, i) do { } while (0)
#define SG_STAMP(i) do { } while (0)
#define SPLIT_STAMP(i) do { } while (0)
#define PROLOGUE_STAMP(i) do { } while (0)
#define ROLL_STAMP(i) do { } while (0)
#define GREEDY_STAMP(i) do { } while (0)
#define POL_STAMP(i) do { } while (0)
#define PROF_ACC(acc, t_prev) nullptr, nullptr
#endif
