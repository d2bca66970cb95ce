#!/usr/bin/env python3
"""Cost of target-selection camera actions (Engine.enable_selection): µs per graph-replayed learner step of
  (a) step_versus_greedy('camera') with the joint action supplied (the flow as it was: the baseline),
  (b) step_selected (executor, step, metrics, restart, action mask),
  (c) the torch route: export_state + a torch restatement of HierarchicalCamera.track + step_versus_greedy,
on MATE-4v8-9 at 4096 and 16 384 environments, frame_skip 1 and 5 (a learner step = frame_skip frames), all three in one process,
interleaved, medians of `--rounds` timed blocks after warm-up.  Prints the table; `--out` also writes it (profiles/selection_probe.txt).

    python tools/selection_probe.py --out profiles/selection_probe.txt
"""
import argparse
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mate_amd.config import read_config, scenario_tables  # noqa: E402
from mate_amd.engine import Engine  # noqa: E402


def torch_track(eng, state, selection, view, out):
    """HierarchicalCamera.track over the batch in torch: state = export_state rows, selection / view [N, Nc, Nt] bool -> out [N, Nc, 2]."""
    f = eng.export_fields
    col = lambda name: state[:, f[name][0]:f[name][0] + eng.num_cameras if name.startswith('cam') else f[name][0] + eng.num_targets]  # noqa: E731
    cam = scenario_tables(eng.config)['camera']
    mva, msr, rot, zoom = cam['min_viewing_angle'], cam['max_sight_range'], cam['rotation_step'], cam['zooming_step']
    valid = (selection & view).to(torch.float64)
    n = valid.sum(-1)
    nn = n.clamp(min=1.0)
    dx = (valid * col('tgt_x')[:, None, :]).sum(-1) / nn - col('cam_x')
    dy = (valid * col('tgt_y')[:, None, :]).sum(-1) / nn - col('cam_y')
    orientation = torch.rad2deg(torch.atan2(dy, dx))
    distance = torch.sqrt(dx * dx + dy * dy).clamp(min=1e-9)
    theta = col('cam_theta')
    area_product = theta * torch.square(torch.sqrt(mva * msr * msr / theta))
    best = torch.full_like(theta, 180.0)
    for _ in range(20):
        best = area_product / torch.square(distance * (1.0 + torch.sin(torch.deg2rad(best.clamp(max=180.0) / 2.0))))
    best = best.clamp(mva, 180.0)
    best = torch.where(distance <= torch.sqrt(area_product / 180.0) / 2.0, torch.full_like(best, 180.0), best)
    best = torch.where(distance * (1.0 + math.sin(math.radians(mva / 2.0))) >= msr, torch.full_like(best, mva), best)
    a0 = (torch.remainder(orientation - col('cam_phi') + 180.0, 360.0) - 180.0).clamp(-rot, rot)
    a1 = (best - theta).clamp(-zoom, zoom)
    some = n > 0
    out[..., 0] = torch.where(some, a0, torch.full_like(a0, -rot))
    out[..., 1] = torch.where(some, a1, torch.full_like(a1, -zoom))


def build(kind, cfg, n, K):
    eng = Engine(cfg, n, seed=1)
    eng.enable_policies()
    eng.reset()
    Nc, Nt = eng.num_cameras, eng.num_targets
    act = torch.zeros((n, Nc, 2), dtype=torch.float64, device=eng.device)
    if kind == 'b':
        eng.enable_selection(True, accumulate=K > 1)
        eng.selection.fill_(0b10110101)
        return eng, eng.make_stepper(None, None, auto_reset=True, graph_steps=4, versus='selection', frame_skip=K)
    between = None
    if kind == 'c':
        state = torch.empty((n, eng.layout.export_width), dtype=torch.float64, device=eng.device)
        selection = ((0b10110101 >> torch.arange(Nt, device=eng.device)) & 1).bool().expand(n, Nc, Nt)
        off = eng.layout.bit_camera_target

        def between():
            eng.export_state(out=state)
            words = eng.masks.to(torch.int64) & 0xffffffff
            bits = ((words[:, :, None] >> torch.arange(32, device=eng.device)) & 1).reshape(n, -1)[:, off:off + Nc * Nt].reshape(n, Nc, Nt).bool()
            torch_track(eng, state, selection, bits, act)
    # frame_skip frames per learner step as per-step launches (the executor acts anew on every frame in (b) and (c); (a) repeats its action)
    return eng, eng.make_stepper(act, None, auto_reset=True, graph_steps=4 * K, between=between, versus='camera')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=200, help='learner steps per timed block')
    ap.add_argument('--out')
    args = ap.parse_args()
    cfg = read_config('MATE-4v8-9.yaml')
    lines = ['MATE-4v8-9, graph-replayed, us per learner step (median [min .. max] of %d blocks of %d learner steps)' % (args.rounds, args.steps),
             '| envs | frame_skip | (a) versus_greedy, actions supplied | (b) step_selected | (c) export_state + torch track | (b) - (a) | (c) / (b) |', '|---|---|---|---|---|---|---|']
    for n in (4096, 16384):
        for K in (1, 5):
            flows = {kind: build(kind, cfg, n, K) for kind in 'abc'}
            times = {kind: [] for kind in 'abc'}
            per = {kind: (args.steps if kind == 'b' else args.steps * K) for kind in 'abc'}
            for kind, (eng, stepper) in flows.items():
                stepper.run(per[kind])                 # warm-up
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for kind, (eng, stepper) in flows.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    stepper.run(per[kind])
                    torch.cuda.synchronize()
                    times[kind].append((time.perf_counter() - t0) / args.steps * 1e6)
            med = {kind: statistics.median(v) for kind, v in times.items()}
            cell = lambda kind: '%.2f [%.2f .. %.2f]' % (med[kind], min(times[kind]), max(times[kind]))  # noqa: E731
            lines.append('| %d | %d | %s | %s | %s | %.2f | %.2f |' % (n, K, cell('a'), cell('b'), cell('c'), med['b'] - med['a'], med['c'] / med['b']))
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
