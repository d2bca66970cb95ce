#!/usr/bin/env python3
"""What the episode records (Engine.enable_episode_records, csrc/episode_rows.hpp) cost a learner; results in profiles/episode_rows_probe.txt.

    python tools/episode_rows_probe.py [--envs 4096 16384] [--reps 5] [--steps 1280]
        Graph-replayed versus='camera' steps (step_versus_greedy) on MATE-4v8-9, us per stepper step, three ways in the SAME process,
        interleaved A B C A B C ...; median and range over the repetitions:
          A  nothing attached beyond what the flow has;
          B  the records attached (camera team): one more launch per step, inside the graph;
          C  the torch equivalent: running sums of the step's scalar record per environment, the episode's
             means written to an [N, 8] tensor where `done`, the sums cleared -- a dozen elementwise operations per step, captured in the
             same graph (the stepper's `between`), which is the cheapest place they can run.
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


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def torch_running_sums(eng):
    """The `between` of mode C: the previous step's record into per-environment running sums, the episode's means out where it ended."""
    n, dev = eng.num_envs, eng.device
    sums = torch.zeros((n, 8), dtype=torch.float64, device=dev)
    steps = torch.zeros(n, dtype=torch.float64, device=dev)
    last = torch.zeros((n, 8), dtype=torch.float64, device=dev)

    def between():
        live, done = eng.scalars[:, 2] != 2, eng.scalars[:, 2] == 1
        record = eng.scalars.double()
        sums.add_(torch.where(live[:, None], record, torch.zeros_like(record)))
        steps.add_(live.double())
        last.copy_(torch.where(done[:, None], sums / steps.clamp(min=1.0)[:, None], last))
        keep = (~done).double()
        sums.mul_(keep[:, None])
        steps.mul_(keep)
    return between, (sums, steps, last)


def main(args):
    has_records = hasattr(Engine, 'enable_episode_records') and not args.detached_only
    modes = ('A', 'B', 'C') if has_records else ('A',)
    print(f'# graph-replayed learner steps on {WORKLOAD}, us per stepper step; A = detached, B = episode records attached (camera team), '
          f'C = torch running sums in the graph; {args.reps} interleaved repetitions, graphs of 64 steps, median [min .. max]')
    for n in args.envs:
        steps = args.steps * (2 if n <= 4096 else 1)
        steppers = {}
        for mode in modes:
            eng = Engine(read_config(WORKLOAD), n, seed=3, obs_dtype=torch.float32)
            eng.enable_policies()
            eng.reset()
            if mode == 'B':
                eng.enable_episode_records('camera')
            between, keep = torch_running_sums(eng) if mode == 'C' else (None, None)
            cam = torch.zeros((n, eng.num_cameras, 2), device='cuda')
            stepper = eng.make_stepper(cam, None, auto_reset=args.versus_interval, graph_steps=64, between=between, versus='camera')
            count = steps
            stepper.run(count)                           # warm-up: every graph replayed, clocks up
            steppers[mode] = (eng, stepper, keep, count)
        times = {mode: [] for mode in steppers}
        for _ in range(args.reps):
            for mode, (eng, stepper, keep, count) in steppers.items():
                times[mode].append(timed(stepper.run, count))
        line = f"N={n:6d} {f'versus=camera, auto_reset={args.versus_interval}':30s}"
        for mode, t in times.items():
            line += f'  {mode} {statistics.median(t):7.2f} [{min(t):7.2f} .. {max(t):7.2f}]'
        if 'B' in times:
            a, b, c = (statistics.median(times[m]) for m in 'ABC')
            line += f'  B - A = {b - a:+.2f} us  C - A = {c - a:+.2f} us'
        print(line, flush=True)
        if 'B' in steppers:
            records, dropped = steppers['B'][0].episode_records()
            print(f'         (B appended {len(records) + dropped} records meanwhile)', flush=True)
        for eng, stepper, keep, count in steppers.values():
            stepper.close()
            eng.close()
        del steppers
        torch.cuda.empty_cache()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, nargs='+', default=[4096, 16384])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=1280)
    ap.add_argument('--detached-only', action='store_true')
    ap.add_argument('--versus-interval', type=int, default=64, help="auto_reset of the versus='camera' flow (bench.py's --versus-reset-interval; 1 = immediate restarts)")
    main(ap.parse_args())
