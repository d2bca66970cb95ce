#!/usr/bin/env python3
"""What routing a learner's messages on the device (Engine.enable_messages / route_messages, csrc/message_rows.hpp) costs; results in
profiles/message_probe.txt.

    python tools/message_probe.py [--envs 4096] [--width 32] [--reps 7] [--steps 1280]
        Graph-replayed versus='camera' steps (step_versus_greedy) on MATE-4v8-9, f32, a target channel with dropout_rate 0.3 and range_limit 1400, us per
        stepper step, three ways in the SAME process, interleaved A B C A B C ...; median and range over the repetitions:
          A  no routing;
          B  the target team's messages ([N, 8, width] per-sender payloads, broadcast) routed by the router launch in front of every step;
          C  the same routing written in torch inside the graph: distances, a uniform per pair, the verdict, the [recipient][sender] inbox by
             torch.where, the per-step edge counts and their two sums (no tags, no totals, positions from a tensor filled once: LESS than B does).
        B - A is the launch's cost in the flow, C - A what a user pays today.
    python tools/message_probe.py --modes B --steps 256 --reps 1      (under rocprofv3 --kernel-trace --stats: the kernel's own time)
    python tools/message_probe.py --roof                              (the library's own write probe, mate_engine_hbm_probe mode 1, GB/s)
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
RATE, LIMIT = 0.3, 1400.0


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def torch_router(eng, width):
    """The routing of mode C as a closure over preallocated tensors."""
    n, N = eng.num_targets, eng.num_envs
    sd = eng.state_dict()
    pos = torch.stack([torch.from_numpy(sd['tgt_x']), torch.from_numpy(sd['tgt_y'])], dim=-1).to(eng.device)      # [N, n, 2] f64
    payload = torch.randn((N, n, width), device=eng.device)
    inbox = torch.zeros((N, n, n, width), device=eng.device)
    step_edges = torch.zeros((N, n, n), dtype=torch.int32, device=eng.device)
    agent_edges = torch.zeros((N, n, 2), dtype=torch.int32, device=eng.device)
    zero = torch.zeros((), device=eng.device)

    def route():
        d = (pos[:, None, :, :] - pos[:, :, None, :]).norm(dim=-1)                 # [sender][recipient]
        u = torch.rand((N, n, n), device=eng.device, dtype=torch.float64)
        keep = (d <= LIMIT) & ~(u > 1.0 - RATE)
        torch.where(keep.transpose(1, 2)[..., None], payload[:, None, :, :], zero, out=inbox)
        step_edges.add_(keep)
        agent_edges.copy_(torch.stack([step_edges.sum(dim=2), step_edges.sum(dim=1)], dim=-1))
    return route, (pos, payload, inbox, step_edges, agent_edges)


def build(mode, n, interval, width):
    eng = Engine(read_config(WORKLOAD), n, seed=3, obs_dtype=torch.float32)
    eng.enable_policies()
    eng.reset()
    eng.set_channel('target', dropout_rate=RATE, range_limit=LIMIT)
    between, keep = None, None
    if mode == 'B':
        payload, _, _ = eng.enable_messages('target', width)
        payload.normal_()
        between = lambda: eng.route_messages('target')      # noqa: E731
    elif mode == 'C':
        between, keep = torch_router(eng, width)
    cam = torch.zeros((n, eng.num_cameras, 2), device='cuda')
    return eng, eng.make_stepper(cam, None, auto_reset=interval, graph_steps=64, versus='camera', between=between), keep


def main(args):
    if args.roof:
        from mate_amd._native import hbm_rates
        print('# mate_engine_hbm_probe, GB/s:', {k: round(v, 1) for k, v in hbm_rates(0).items()})
        return
    print(f'# graph-replayed learner steps on {WORKLOAD}, f32, target channel (rate {RATE}, range {LIMIT:g}), messages of {args.width} numbers, us per stepper step; '
          f'A = no routing, B = the router launch, C = the same routing in torch; {args.reps} interleaved repetitions, graphs of 64 steps, median [min .. max]')
    for n in args.envs:
        steppers = {mode: build(mode, n, args.versus_interval, args.width) for mode in args.modes}
        for eng, stepper, _ in steppers.values():
            stepper.run(args.steps)                      # warm-up: every graph replayed, clocks up
        times = {mode: [] for mode in steppers}
        for _ in range(args.reps):
            for mode, (eng, stepper, _) in steppers.items():
                times[mode].append(timed(stepper.run, args.steps))
        inbox_mb = n * eng.num_targets ** 2 * args.width * 4 / 1e6
        line = f"N={n:6d} versus=camera, auto_reset={args.versus_interval}, inbox {inbox_mb:.1f} MB"
        for mode, t in times.items():
            line += f'  {mode} {statistics.median(t):7.2f} [{min(t):7.2f} .. {max(t):7.2f}]'
        if all(m in times for m in 'ABC'):
            a, b, c = (statistics.median(times[m]) for m in 'ABC')
            line += f'  B - A = {b - a:+.2f} us  C - A = {c - a:+.2f} us'
        print(line, flush=True)
        for eng, stepper, _ in steppers.values():
            stepper.close()
            eng.close()
        del steppers
        torch.cuda.empty_cache()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, nargs='+', default=[4096])
    ap.add_argument('--width', type=int, default=32)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--steps', type=int, default=1280)
    ap.add_argument('--modes', default='ABC', help='which of A, B, C to run')
    ap.add_argument('--versus-interval', type=int, default=64, help="auto_reset of the versus='camera' flow (1 = immediate restarts)")
    ap.add_argument('--roof', action='store_true', help='print the write rate of mate_engine_hbm_probe and exit')
    main(ap.parse_args())
