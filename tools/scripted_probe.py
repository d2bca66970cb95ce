#!/usr/bin/env python3
"""What an opponent mixture (Engine.set_opponent_mixture, csrc/scripted_rows.hpp) costs a learner; results in profiles/scripted_probe.txt.

    python tools/scripted_probe.py [--envs 4096] [--reps 5] [--steps 1280]
        Graph-replayed versus='camera' steps (step_versus_greedy) on MATE-4v8-9, us per stepper step, three ways in the SAME process,
        interleaved A B C A B C ...; median and range over the repetitions:
          A  no mixture: the Greedy targets, the one-launch form of the flow;
          B  {naive: 1}: the scripted launch and the stepping launch -- no Greedy agents' launch, nobody needs their row;
          C  {greedy, naive, random}: the Greedy agents' launch (for every environment, whatever its choice), the scripted launch, the
             stepping launch.
        The per-step flow only: the FrameSkip flow is not measured.
        `--detached-only` runs A alone: from a checkout of the parent commit its figures must agree with this commit's A.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mate_amd.config import read_config  # noqa: E402
from mate_amd.engine import Engine  # noqa: E402

WORKLOAD = 'MATE-4v8-9.yaml'
MIXTURES = {'A': None, 'B': {'naive': 1.0}, 'C': {'greedy': 1.0, 'naive': 1.0, 'random': 1.0}}


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def main(args):
    has_mixtures = hasattr(Engine, 'set_opponent_mixture') and not args.detached_only
    modes = ('A', 'B', 'C') if has_mixtures else ('A',)
    print(f'# graph-replayed learner steps on {WORKLOAD}, us per stepper step; A = no mixture, B = target mixture {{naive}}, '
          f'C = target mixture {{greedy, naive, random}}; {args.reps} interleaved repetitions, graphs of 64 steps, median [min .. max]')
    for n in args.envs:
        steps = args.steps * (2 if n <= 4096 else 1)
        steppers = {}
        for mode in modes:
            eng = Engine(read_config(WORKLOAD), n, seed=3, obs_dtype=torch.float32)
            eng.enable_policies()
            eng.reset()
            if MIXTURES[mode] is not None:
                eng.set_opponent_mixture('target', MIXTURES[mode])
            cam = torch.zeros((n, eng.num_cameras, 2), device='cuda')
            stepper = eng.make_stepper(cam, None, auto_reset=args.versus_interval, graph_steps=64, versus='camera')
            stepper.run(steps)                           # warm-up: every graph replayed, clocks up
            steppers[mode] = (eng, stepper)
        times = {mode: [] for mode in steppers}
        for _ in range(args.reps):
            for mode, (eng, stepper) in steppers.items():
                times[mode].append(timed(stepper.run, steps))
        line = f"N={n:6d} {f'versus=camera, auto_reset={args.versus_interval}':30s}"
        for mode, t in times.items():
            line += f'  {mode} {statistics.median(t):7.2f} [{min(t):7.2f} .. {max(t):7.2f}]'
        if 'C' in times:
            a, b, c = (statistics.median(times[m]) for m in 'ABC')
            line += f'  B - A = {b - a:+.2f} us  C - A = {c - a:+.2f} us'
        print(line, flush=True)
        for eng, stepper in steppers.values():
            stepper.close()
            eng.close()
        del steppers
        torch.cuda.empty_cache()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, nargs='+', default=[4096])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=1280)
    ap.add_argument('--detached-only', action='store_true')
    ap.add_argument('--versus-interval', type=int, default=64, help="auto_reset of the versus='camera' flow (bench.py's --versus-reset-interval; 1 = immediate restarts)")
    main(ap.parse_args())
