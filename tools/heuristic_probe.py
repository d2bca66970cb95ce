#!/usr/bin/env python3
"""Cost of the Heuristic target opponent (Engine.set_target_opponent): µs per graph-replayed
step_versus_greedy('camera') of MATE-4v8-9 at 4096 and 16 384 environments (graphs of 64 steps, batched restarts every 32) in three forms,
  (a) Greedy targets, the one-launch form (agents and step in one kernel),
  (b) Greedy targets, the two-launch form (MATE_POLICY_SPLIT=1: agents' launch, stepping launch),
  (c) Heuristic targets: agents' launch, drift launch, stepping launch,
all three in one process, interleaved; `--series` repeated series of `--rounds` timed blocks give the run-to-run spread next to the
medians.  (c) - (b) is the drift launch, (b) - (a) what leaving the one-launch form costs.  Prints the table; `--out` also writes it
(profiles/heuristic_probe.txt).

    python tools/heuristic_probe.py --out profiles/heuristic_probe.txt
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

LEGS = 'abc'
GRAPH_STEPS, RESET_INTERVAL = 64, 32      # (the learner flows' setting: batched restarts, whole intervals per graph)


def build(kind, cfg, n):
    if kind == 'b':
        os.environ['MATE_POLICY_SPLIT'] = '1'      # (read once, at create)
    try:
        eng = Engine(cfg, n, seed=1)
    finally:
        os.environ.pop('MATE_POLICY_SPLIT', None)
    eng.enable_policies(target_agent='heuristic' if kind == 'c' else 'greedy')
    eng.reset()
    act = torch.zeros((n, eng.num_cameras, 2), dtype=torch.float32, device=eng.device)
    stepper = eng.make_stepper(act, None, auto_reset=RESET_INTERVAL, graph_steps=GRAPH_STEPS, versus='camera')
    return eng, stepper


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--series', type=int, default=3)
    ap.add_argument('--steps', type=int, default=640, help='steps per timed block (a multiple of %d)' % GRAPH_STEPS)
    ap.add_argument('--out')
    args = ap.parse_args()
    assert args.steps % GRAPH_STEPS == 0
    lines = ['MATE-4v8-9, step_versus_greedy(camera), graph-replayed (graphs of %d steps, batched restarts every %d), us per step: median over %d series x %d blocks of %d steps [min .. max of the series medians]'
             % (GRAPH_STEPS, RESET_INTERVAL, args.series, args.rounds, args.steps),
             '| envs | (a) Greedy, one launch | (b) Greedy, two launches | (c) Heuristic, three launches | (b) - (a) | (c) - (b) |', '|---|---|---|---|---|---|']
    cfg = read_config('MATE-4v8-9.yaml')
    for n in (4096, 16384):
        flows = {kind: build(kind, cfg, n) for kind in LEGS}
        for eng, stepper in flows.values():
            stepper.run(args.steps)      # warm-up
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
        cell = lambda kind: '%.2f [%.2f .. %.2f]' % (med[kind], min(medians[kind]), max(medians[kind]))  # noqa: E731
        lines.append('| %d | %s | %s | %s | %.2f | %.2f |' % (n, cell('a'), cell('b'), cell('c'), med['b'] - med['a'], med['c'] - med['b']))
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
