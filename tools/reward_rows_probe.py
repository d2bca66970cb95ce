#!/usr/bin/env python3
"""What a learner pays for shaped rewards (Engine.enable_reward_rows, csrc/reward_rows.hpp); results in profiles/reward_rows_probe.txt.

    python tools/reward_rows_probe.py [--envs 4096 16384] [--reps 5] [--steps 2000] [--out FILE]

End-to-end us per step of step_versus_greedy('target') on MATE-2v4-0 and step_versus_greedy('camera') on MATE-4v8-9 with the example
trainers' coefficient sets (examples/ippo/target/config.py: five target terms, 'none'; examples/ippo/camera/config.py:
coverage_rate, 'mean'), batched restarts every 64th step, four ways on the same process, interleaved over the repetitions:

    unshaped   the step alone, direct calls
    torch      ... followed by the torch shaper (BatchedMultiAgentTracking.auxiliary_*_rewards), direct calls
    attached   the reward launch attached, direct calls
    graph      unshaped / attached, replayed from HIP graphs of 64 steps (the torch shaper allocates: it cannot be captured)

Every figure: a host clock around `steps` steps that end in a device synchronise, after a warm-up of the same length; median
[min .. max] over the repetitions.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mate_amd.environment import BatchedMultiAgentTracking  # noqa: E402

INTERVAL = 64
POINTS = {
    'target': ('MATE-2v4-0.yaml', {'raw_reward': 1.0, 'normalized_goal_distance': -0.5, 'is_tracked': -0.25, 'is_colliding': -1.0, 'sparse_delivery': 5.0}, 'none'),
    'camera': ('MATE-4v8-9.yaml', {'coverage_rate': 1.0}, 'mean'),
}


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def make(team, n, attached):
    config, coefficients, reduction = POINTS[team]
    env = BatchedMultiAgentTracking(config, num_envs=n, seed=3, auto_reset=INTERVAL,
                                    **({f'{team}_reward_shaping': (coefficients, reduction)} if attached else {}))
    env.enable_greedy_policies()
    env.reset()
    agents = env.num_cameras if team == 'camera' else env.num_targets
    return env, torch.zeros((n, agents, 2), device='cuda')


def main(args):
    lines = [f'# us per step, end to end; batched restarts every {INTERVAL}th step; {args.reps} interleaved repetitions of {args.steps} steps, median [min .. max]']
    for team in ('target', 'camera'):
        config, coefficients, reduction = POINTS[team]
        for n in args.envs:
            plain, act_p = make(team, n, False)
            shaped, act_s = make(team, n, True)
            torch_env, act_t = make(team, n, False)
            torch_shaper = torch_env.auxiliary_camera_rewards if team == 'camera' else torch_env.auxiliary_target_rewards

            def direct(env, act, after=None):
                def run(steps):
                    for _ in range(steps):
                        env.engine.step_versus_greedy(team, act, auto_reset=INTERVAL)
                        if after is not None:
                            after(coefficients, reduction)
                return run
            ways = {'unshaped': direct(plain, act_p), 'torch': direct(torch_env, act_t, torch_shaper), 'attached': direct(shaped, act_s)}
            times = {way: [] for way in ways}
            for way, run in ways.items():
                run(args.steps)                                   # warm-up
            for _ in range(args.reps):
                for way, run in ways.items():
                    times[way].append(timed(run, args.steps))
            # the same two engines, now replayed from graphs (the constructor runs one whole interval first)
            steppers = {'graph unshaped': plain.engine.make_stepper(act_p if team == 'camera' else None, act_p if team == 'target' else None,
                                                                     auto_reset=INTERVAL, graph_steps=INTERVAL, versus=team),
                        'graph attached': shaped.engine.make_stepper(act_s if team == 'camera' else None, act_s if team == 'target' else None,
                                                                     auto_reset=INTERVAL, graph_steps=INTERVAL, versus=team)}
            steps = args.steps // INTERVAL * INTERVAL
            for way, stepper in steppers.items():
                times[way] = []
                stepper.run(steps)
            for _ in range(args.reps):
                for way, stepper in steppers.items():
                    times[way].append(timed(stepper.run, steps))
            med = {way: statistics.median(t) for way, t in times.items()}
            line = f'{config[:-5]:11s} versus={team:6s} N={n:6d}'
            for way, t in times.items():
                line += f'  {way} {med[way]:7.2f} [{min(t):7.2f} .. {max(t):7.2f}]'
            line += (f"  | attached - unshaped = {med['attached'] - med['unshaped']:.2f} (graph {med['graph attached'] - med['graph unshaped']:.2f}), "
                     f"torch - unshaped = {med['torch'] - med['unshaped']:.2f}, attached / torch = {med['attached'] / med['torch']:.3f}")
            print(line, flush=True)
            lines.append(line)
            for stepper in steppers.values():
                stepper.close()
            for env in (plain, shaped, torch_env):
                env.close()
            del steppers, ways, plain, shaped, torch_env
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, nargs='+', default=[4096, 16384])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=1920)
    ap.add_argument('--out', default=None)
    main(ap.parse_args())
