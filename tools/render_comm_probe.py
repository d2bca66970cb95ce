#!/usr/bin/env python3
"""Cost of the communication trace and of its arrows, ONE engine and ONE process per measurement:

    python tools/render_comm_probe.py render none|empty|full   # 12 render launches of 8 environments at 800 x 800 and at 200 x 200 -- without a trace, with an
                                                               #   all-zero one, with every pair live: run each under
                                                               #   rocprofv3 --kernel-trace --stats -d DIR -- python tools/render_comm_probe.py render full
    python tools/render_comm_probe.py trace                    # 200 step_greedy calls with the trace attached, under rocprofv3 likewise: comm_trace_kernel's row
    python tools/render_comm_probe.py step trace|plain         # ONE graph-replayed stepper (versus='camera', 4096 environments, the targets' transparent channel)
                                                               #   with and -- in a process of its own -- without the trace: host clock per replayed step

MATE-8v8-9, 8 environments, 60 steps under the on-device Greedy agents of both teams for the render cases: 3.20's setting."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mate_amd.config import read_config  # noqa: E402
from mate_amd.engine import Engine  # noqa: E402

ENVS, SIZES = 8, (800, 200)


def render(mode):
    eng = Engine(read_config('MATE-8v8-9.yaml'), ENVS, seed=0)
    eng.enable_policies()
    eng.reset()
    for _ in range(60):
        eng.step_greedy(auto_reset=1)
    if mode != 'none':
        eng.enable_communication_trace(duration=20)
        for team, n in enumerate((eng.num_cameras, eng.num_targets)):
            eng.set_communication_trace(team, np.full((ENVS, n, n), 20 if mode == 'full' else 0, dtype=np.uint8))
    torch.cuda.synchronize()
    for size in SIZES:
        out = torch.empty((ENVS, size, size, 3), dtype=torch.uint8, device=eng.device)
        for _ in range(12):
            eng.render(size=size, out=out)
    torch.cuda.synchronize()
    print('render', mode, ': 12 launches per size', SIZES, 'of', ENVS, 'environments: read the kernel statistics')


def trace():
    eng = Engine(read_config('MATE-8v8-9.yaml'), 4096, seed=0)
    eng.enable_policies()
    eng.reset()
    eng.enable_communication_trace(duration=20)
    for _ in range(200):
        eng.step_greedy(auto_reset=1)
    torch.cuda.synchronize()
    print('trace: 200 step_greedy calls of 4096 environments with the trace attached: read comm_trace_kernel in the kernel statistics')


def step(mode):
    n, K = 4096, 16
    eng = Engine(read_config('MATE-8v8-9.yaml'), n, seed=0)
    eng.enable_policies()
    eng.reset()
    eng.set_channel('target')
    if mode == 'trace':
        eng.enable_communication_trace(teams=('target',), duration=20)
    action = torch.zeros((n, eng.num_cameras, 2), dtype=torch.float64, device=eng.device)
    stepper = eng.make_stepper(action, None, auto_reset=K, graph_steps=K, versus='camera')
    stepper.run(4 * K)
    torch.cuda.synchronize()
    times = []
    for _ in range(10):
        t0 = time.perf_counter()
        stepper.run(8 * K)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / (8 * K) * 1e6)
    print(f'step {mode}: graph-replayed step_versus_greedy(camera) of {n} x MATE-8v8-9, us per step: median {np.median(times):.2f}, min {min(times):.2f}, max {max(times):.2f} (10 runs of {8 * K} steps)')
    stepper.close()


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'render'
    if what == 'render':
        render(sys.argv[2] if len(sys.argv) > 2 else 'full')
    elif what == 'trace':
        trace()
    else:
        step(sys.argv[2] if len(sys.argv) > 2 else 'trace')
