#!/usr/bin/env python3
"""Measurements of the global state rows (Engine.enable_state_rows, csrc/state_rows.hpp); results in profiles/state_rows_probe.txt.

    python tools/state_rows_probe.py learner [--envs 4096 16384 65536] [--reps 5]
        What a learner pays: graph-replayed step(actions) and versus='camera' steps on MATE-4v8-9, us per step with the rows detached
        (A) and attached (B, f32 normalised), the SAME process and engines, interleaved A B A B ...; median and range over the repetitions.
        Run it from a checkout of the parent commit as well (`learner --detached-only`): the detached figures of the two must agree.
    python tools/state_rows_probe.py copy [--envs 65536]
        The memory system's yardstick: mate_engine_hbm_probe's copy mode over as many bytes as one state launch moves (records read +
        rows written, counted from the layout), against device-event times of the launch itself.
    python tools/state_rows_probe.py kernel [--envs 65536] [--launches 200]
        The body to profile: `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/state_rows_probe.py kernel` (a run of its own).
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mate_amd import _native  # noqa: E402
from mate_amd.config import read_config  # noqa: E402
from mate_amd.engine import Engine  # noqa: E402

WORKLOAD = 'MATE-4v8-9.yaml'


def layout_bytes(eng, row_size=4):
    """(record bytes read, row bytes written) of one state launch, from the layout: SW + DW 8-byte record words, state_dim reals."""
    Nc, Nt, No = eng.num_cameras, eng.num_targets, eng.num_obstacles
    sw = 3 * Nc + 3 * No + 1
    ni = Nt * 5 + 26
    dw = 2 * Nc + 2 * Nt + 2 + (ni + (ni & 1)) // 2
    return eng.num_envs * (sw + dw) * 8, eng.num_envs * eng.state_dim * row_size


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def learner(args):
    has_rows = hasattr(Engine, 'enable_state_rows') and not args.detached_only
    print(f'# graph-replayed steps on {WORKLOAD}, us per step; A = rows detached, B = rows attached (f32, normalised); '
          f'{args.reps} interleaved repetitions of {args.steps} (65 536 environments) .. {4 * args.steps} (4096) steps each (graphs of 64), median [min .. max]')
    for n in args.envs:
        steps = args.steps * (4 if n <= 4096 else 2 if n <= 16384 else 1)      # (a timed window of a few tenths of a second at every size)
        for versus in [v for v, name in ((None, 'step'), ('camera', 'versus')) if name in args.flows]:
            steppers = {}
            for mode in ('A', 'B') if has_rows else ('A',):
                eng = Engine(read_config(WORKLOAD), n, seed=3, obs_dtype=torch.float32)
                if versus:
                    eng.enable_policies()
                eng.reset()
                if mode == 'B':
                    eng.enable_state_rows(normalize=True)
                cam = torch.zeros((n, eng.num_cameras, 2), device='cuda')
                tgt = torch.zeros((n, eng.num_targets, 2), device='cuda')
                stepper = eng.make_stepper(cam, tgt, auto_reset=args.versus_interval if versus else True, graph_steps=64, versus=versus)
                stepper.run(steps)                           # warm-up: every graph replayed, clocks up
                steppers[mode] = (eng, stepper)
            times = {mode: [] for mode in steppers}
            for _ in range(args.reps):
                for mode, (eng, stepper) in steppers.items():
                    times[mode].append(timed(stepper.run, steps))
            line = f"N={n:6d} {'step(actions), auto_reset=1' if versus is None else f'versus=camera, auto_reset={args.versus_interval}':30s}"
            for mode, t in times.items():
                line += f'  {mode} {statistics.median(t):7.2f} [{min(t):7.2f} .. {max(t):7.2f}]'
            if 'B' in times:
                a, b = statistics.median(times['A']), statistics.median(times['B'])
                line += f'  attached / detached = {b / a:.3f}'
            print(line, flush=True)
            for eng, stepper in steppers.values():
                stepper.close()
                eng.close()
            del steppers
            torch.cuda.empty_cache()


def copy(args):
    n = args.envs[0]
    eng = Engine(read_config(WORKLOAD), n, seed=3, obs_dtype=torch.float32)
    eng.reset()
    state = eng.enable_state_rows(normalize=True)
    eng.disable_state_rows()
    read_b, write_b = layout_bytes(eng)
    print(f'# one state launch at N = {n}: {read_b} record bytes read + {write_b} row bytes written = {read_b + write_b} bytes')
    # the copy yardstick over the same number of bytes (read + written): a copy of `half` bytes reads half and writes half
    half = (read_b + write_b) // 2 // 16 * 16
    a = torch.zeros(half, dtype=torch.uint8, device='cuda')
    b = torch.zeros(half, dtype=torch.uint8, device='cuda')
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rates = []
    for _ in range(args.reps):
        rate = ctypes.c_double()
        _native.check(eng.lib.mate_engine_hbm_probe(0, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), half, 0, stream, ctypes.byref(rate)))
        rates.append(rate.value)
    copy_us = [2 * half / (r * 1e9) * 1e6 for r in rates]
    print(f'hbm_probe copy of 2 x {half} bytes: {statistics.median(rates):.0f} GB/s [{min(rates):.0f} .. {max(rates):.0f}] = '
          f'{statistics.median(copy_us):.2f} us [{min(copy_us):.2f} .. {max(copy_us):.2f}] (each the median of five launches)')
    big = _native.hbm_rates(0, gib=1.0)
    print(f"hbm_probe over 1 GiB buffers: copy {big['copy']:.0f} GB/s -> {(read_b + write_b) / (big['copy'] * 1e9) * 1e6:.2f} us for the same bytes at that rate")
    for _ in range(20):
        eng.state_rows(out=state, normalize=True)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.launches)]
    for e0, e1 in ev:
        e0.record()
        eng.state_rows(out=state, normalize=True)
        e1.record()
    torch.cuda.synchronize()
    us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
    print(f'state_rows launch (f32, normalised), device events around single launches (marker latency included), {args.launches} launches: '
          f'median {statistics.median(us):.2f} us, min {us[0]:.2f}, p90 {us[int(0.9 * len(us))]:.2f}')
    # back to back: launches queue up behind each other, the average is the kernel's own duration plus the dispatch gap
    t = timed(lambda k: [eng.state_rows(out=state, normalize=True) for _ in range(k)], 2000)
    print(f'2000 launches back to back: {t:.2f} us per launch = {(read_b + write_b) / t / 1e3:.0f} GB/s of the layout bytes')


def kernel(args):
    n = args.envs[0]
    eng = Engine(read_config(WORKLOAD), n, seed=3, obs_dtype=torch.float32)
    eng.reset()
    state = eng.enable_state_rows(normalize=True)
    eng.disable_state_rows()
    for _ in range(args.launches):
        eng.state_rows(out=state, normalize=True)
    torch.cuda.synchronize()
    print(f'{args.launches} state launches at N = {n}: bytes per launch {sum(layout_bytes(eng))}')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['learner', 'copy', 'kernel'])
    ap.add_argument('--envs', type=int, nargs='+', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=6400)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--detached-only', action='store_true')
    ap.add_argument('--versus-interval', type=int, default=64, help="auto_reset of the versus='camera' flow (bench.py's --versus-reset-interval; 1 = immediate restarts)")
    ap.add_argument('--flows', nargs='+', default=['step', 'versus'], choices=['step', 'versus'])
    args = ap.parse_args()
    if args.envs is None:
        args.envs = [4096, 16384, 65536] if args.mode == 'learner' else [65536]
    {'learner': learner, 'copy': copy, 'kernel': kernel}[args.mode](args)
