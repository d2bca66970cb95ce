#!/usr/bin/env python3
"""What a communication channel (Engine.set_channel, csrc/channel_rows.hpp) costs a learner; results in profiles/channel_probe.txt.

    python tools/channel_probe.py [--envs 4096] [--reps 7] [--steps 1280]
        Graph-replayed versus='camera' steps (step_versus_greedy) on MATE-4v8-9, us per stepper step, three ways in the SAME process,
        interleaved A B C A B C ...; median and range over the repetitions:
          A  no channel: the one-launch form of the flow (what a channel takes a step away from -- the cost of MATE_POLICY_SPLIT=1, not the channel's);
          B  no channel, MATE_POLICY_SPLIT=1: the two-launch form with the scenario's SPECIALISED greedy_policy_kernel -- the point of reference
             (no existing kernel differs from the parent commit's: this is the parent's split form);
          C  a target channel with dropout_rate 0.3: the two-launch form with the generic-shape greedy_channel_kernel in the agents' launch's place.
        C - B is the channel's own cost: the verdicts and the edge rows, and whatever the generic shape loses to the specialised one.
    python tools/channel_probe.py --modes C --steps 256 --reps 1      (under rocprofv3 --kernel-trace --stats: the kernels' own times)
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


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def build(mode, n, interval):
    if mode == 'B':
        os.environ['MATE_POLICY_SPLIT'] = '1'      # (read once, at create)
    try:
        eng = Engine(read_config(WORKLOAD), n, seed=3, obs_dtype=torch.float32)
    finally:
        os.environ.pop('MATE_POLICY_SPLIT', None)
    eng.enable_policies()
    eng.reset()
    if mode == 'C':
        eng.set_channel('target', dropout_rate=0.3)
    cam = torch.zeros((n, eng.num_cameras, 2), device='cuda')
    return eng, eng.make_stepper(cam, None, auto_reset=interval, graph_steps=64, versus='camera')


def main(args):
    print(f'# graph-replayed learner steps on {WORKLOAD}, us per stepper step; A = one launch, B = two launches (specialised agents\' kernel), '
          f'C = two launches with a target channel (rate 0.3); {args.reps} interleaved repetitions, graphs of 64 steps, median [min .. max]')
    for n in args.envs:
        steppers = {mode: build(mode, n, args.versus_interval) for mode in args.modes}
        for eng, stepper in steppers.values():
            stepper.run(args.steps)                      # warm-up: every graph replayed, clocks up
        times = {mode: [] for mode in steppers}
        for _ in range(args.reps):
            for mode, (eng, stepper) in steppers.items():
                times[mode].append(timed(stepper.run, args.steps))
        line = f"N={n:6d} versus=camera, auto_reset={args.versus_interval}"
        for mode, t in times.items():
            line += f'  {mode} {statistics.median(t):7.2f} [{min(t):7.2f} .. {max(t):7.2f}]'
        if all(m in times for m in 'ABC'):
            a, b, c = (statistics.median(times[m]) for m in 'ABC')
            line += f'  B - A = {b - a:+.2f} us  C - B = {c - b:+.2f} us'
        print(line, flush=True)
        for eng, stepper in steppers.values():
            stepper.close()
            eng.close()
        del steppers
        torch.cuda.empty_cache()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, nargs='+', default=[4096])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--steps', type=int, default=1280)
    ap.add_argument('--modes', default='ABC', help='which of A, B, C to run')
    ap.add_argument('--versus-interval', type=int, default=64, help="auto_reset of the versus='camera' flow (1 = immediate restarts)")
    main(ap.parse_args())
