#!/usr/bin/env python3
"""What the training-information rows (Engine.enable_info_rows, csrc/info_rows.hpp) cost a learner; results in profiles/info_rows_probe.txt.

    python tools/info_rows_probe.py [--envs 4096] [--reps 5] [--steps 1280]
        Graph-replayed versus='camera' steps (step_versus_greedy) on MATE-4v8-9, us per stepper step, three ways in the SAME process,
        interleaved A B C A B C ...; median and range over the repetitions:
          A  nothing attached beyond what the flow has;
          B  the rows attached (all three outputs): one more launch per step, inside the graph;
          C  the torch equivalent: the same columns from the engine's dynamic records (Engine.export_state) and the packed mask words --
             an export launch, the unpacking shifts, the four distances, the comparison with a kept copy of the goals -- captured in the
             same graph (the stepper's `between`), which is the cheapest place they can run.  It describes the state BEHIND the restart:
             what torch cannot see (the terminal step under auto_reset = 1) costs nothing here.
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
WAREHOUSES = ((925.0, 925.0), (-925.0, 925.0), (-925.0, -925.0), (925.0, -925.0))


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def torch_info(eng):
    """The `between` of mode C: the rows of the previous step's records with torch operations on the exported state and the mask words."""
    n, nc, nt, dev = eng.num_envs, eng.num_cameras, eng.num_targets, eng.device
    fields = eng.export_fields
    flat = torch.zeros((n, eng.layout.export_width), dtype=torch.float64, device=dev)
    target = torch.zeros((n, nt, 9), dtype=torch.float64, device=dev)
    camera = torch.zeros((n, nc, 2), dtype=torch.float64, device=dev)
    cargo = torch.zeros((n, 24), dtype=torch.float64, device=dev)
    goals_before = torch.full((n, nt), -1.0, dtype=torch.float64, device=dev)
    centres = torch.tensor(WAREHOUSES, dtype=torch.float64, device=dev)
    ct_bits = torch.arange(nc * nt, device=dev) + eng.layout.bit_camera_target
    tc_bits = (eng.layout.bit_target_row + torch.arange(nt, device=dev)[:, None] * (nc + eng.num_obstacles + nt) + torch.arange(nc, device=dev)[None, :]).reshape(-1)

    def column(name, width):
        off = fields[name][0]
        return flat[:, off:off + width]

    def between():
        eng.export_state(out=flat)
        words = eng.masks.long()
        ct = ((words[:, ct_bits // 32] >> (ct_bits % 32)) & 1).view(n, nc, nt)
        tc = ((words[:, tc_bits // 32] >> (tc_bits % 32)) & 1).view(n, nt, nc)
        goals = column('tgt_goals', nt)
        xy = torch.stack((column('tgt_x', nt), column('tgt_y', nt)), dim=-1)
        d = xy[:, :, None, :] - centres
        wd = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).sqrt() - 75.0).clamp(min=0.0)
        target[:, :, 0] = goals
        target[:, :, 1] = torch.where(goals >= 0, wd.gather(2, goals.clamp(min=0).long()[..., None])[..., 0], torch.full_like(goals, 1000.0))
        target[:, :, 2:6] = wd
        target[:, :, 6] = ((goals != goals_before) & (goals_before >= 0)).double()
        target[:, :, 7] = ct.any(dim=1).double()
        target[:, :, 8] = column('tgt_colliding', nt)
        camera[:, :, 0] = ct.sum(dim=2).double()
        camera[:, :, 1] = tc.any(dim=1).double()
        remaining = column('remaining_cargoes', 16)
        cargo[:, 0:4] = remaining.view(n, 4, 4).sum(dim=2)
        cargo[:, 4:8] = column('awaiting_cargo_counts', 4)
        cargo[:, 8:24] = remaining
        goals_before.copy_(goals)
    return between, (flat, target, camera, cargo, goals_before)


def main(args):
    has_rows = hasattr(Engine, 'enable_info_rows') and not args.detached_only
    modes = ('A', 'B', 'C') if has_rows else ('A',)
    print(f'# graph-replayed learner steps on {WORKLOAD}, us per stepper step; A = detached, B = training-information rows attached, '
          f'C = the torch equivalent in the graph; {args.reps} interleaved repetitions, graphs of 64 steps, median [min .. max]')
    for n in args.envs:
        steps = args.steps * (2 if n <= 4096 else 1)
        steppers = {}
        for mode in modes:
            eng = Engine(read_config(WORKLOAD), n, seed=3, obs_dtype=torch.float32)
            eng.enable_policies()
            eng.reset()
            if mode == 'B':
                eng.enable_info_rows()
            between, keep = torch_info(eng) if mode == 'C' else (None, None)
            cam = torch.zeros((n, eng.num_cameras, 2), device='cuda')
            stepper = eng.make_stepper(cam, None, auto_reset=args.versus_interval, graph_steps=64, between=between, versus='camera')
            stepper.run(steps)                           # warm-up: every graph replayed, clocks up
            steppers[mode] = (eng, stepper, keep)
        times = {mode: [] for mode in steppers}
        for _ in range(args.reps):
            for mode, (eng, stepper, keep) in steppers.items():
                times[mode].append(timed(stepper.run, steps))
        line = f"N={n:6d} {f'versus=camera, auto_reset={args.versus_interval}':30s}"
        for mode, t in times.items():
            line += f'  {mode} {statistics.median(t):7.2f} [{min(t):7.2f} .. {max(t):7.2f}]'
        if 'B' in times:
            a, b, c = (statistics.median(times[m]) for m in 'ABC')
            line += f'  B - A = {b - a:+.2f} us  C - A = {c - a:+.2f} us'
        print(line, flush=True)
        for eng, stepper, keep in steppers.values():
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
