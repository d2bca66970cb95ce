#!/usr/bin/env python3
"""Cost of the Heuristic camera opponent (Engine.set_camera_opponent): µs per graph-replayed
step_versus_greedy('target') at MATE-4v8-9 x 4096 and MATE-2v4-0 x 16 384 (graphs of 64 steps, batched restarts every 32) in two forms,
  (a) Greedy cameras, the one-launch form (agents and step in one kernel) -- the flow as it was before this opponent existed,
  (b) Heuristic cameras: heuristic_camera_kernel, stepping launch,
both in one process, interleaved; `--series` repeated series of `--rounds` timed blocks give the run-to-run spread next to the medians.
Prints the table; `--out` also writes it (profiles/heuristic_camera_probe.txt).

    python tools/heuristic_camera_probe.py --out profiles/heuristic_camera_probe.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mate_amd.config import read_config  # noqa: E402
from mate_amd.engine import Engine  # noqa: E402

LEGS = 'ab'
GRAPH_STEPS, RESET_INTERVAL = 64, 32      # (the learner flows' setting: batched restarts, whole intervals per graph)
SHAPES = (('MATE-4v8-9.yaml', 4096), ('MATE-2v4-0.yaml', 16384))


def build(kind, cfg, n):
    eng = Engine(cfg, n, seed=1)
    eng.enable_policies(camera_agent='heuristic' if kind == 'b' else 'greedy')
    eng.reset()
    act = torch.zeros((n, eng.num_targets, 2), dtype=torch.float32, device=eng.device)
    stepper = eng.make_stepper(None, act, auto_reset=RESET_INTERVAL, graph_steps=GRAPH_STEPS, versus='target')
    return eng, stepper


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--series', type=int, default=3)
    ap.add_argument('--steps', type=int, default=128, help='steps per timed block (a multiple of %d)' % GRAPH_STEPS)
    ap.add_argument('--out')
    args = ap.parse_args()
    assert args.steps % GRAPH_STEPS == 0
    lines = ['step_versus_greedy(target), graph-replayed (graphs of %d steps, batched restarts every %d), us per step: median over %d series x %d blocks of %d steps [min .. max of the series medians]'
             % (GRAPH_STEPS, RESET_INTERVAL, args.series, args.rounds, args.steps),
             '| scenario | envs | (a) Greedy cameras, one launch | (b) Heuristic cameras, two launches | (b) - (a) | (b) / (a) |', '|---|---|---|---|---|---|']
    for config, n in SHAPES:
        cfg = read_config(config)
        flows = {kind: build(kind, cfg, n) for kind in LEGS}
        for eng, stepper in flows.values():
            stepper.run(GRAPH_STEPS)      # warm-up
        torch.cuda.synchronize()
        medians = {kind: [] for kind in LEGS}
        for _ in range(args.series):
            times = {kind: [] for kind in LEGS}
            for _ in range(args.rounds):
                for kind, (eng, stepper) in flows.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    stepper.run(args.steps)
                    torch.cuda.synchronize()
                    times[kind].append((time.perf_counter() - t0) / args.steps * 1e6)
            for kind in LEGS:
                medians[kind].append(statistics.median(times[kind]))
        med = {kind: statistics.median(v) for kind, v in medians.items()}
        cell = lambda kind: '%.1f [%.1f .. %.1f]' % (med[kind], min(medians[kind]), max(medians[kind]))  # noqa: E731
        lines.append('| %s | %d | %s | %s | %.1f | %.1f |' % (config[:-5], n, cell('a'), cell('b'), med['b'] - med['a'], med['b'] / med['a']))
        for eng, stepper in flows.values():
            stepper.close()
            eng.close()
        print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
