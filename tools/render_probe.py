#!/usr/bin/env python3
"""Cost of the off-screen render, one engine and one process per measurement:

    python tools/render_probe.py kernel     # a few render launches of 8 environments at 800 x 800 and at 200 x 200: run it under
                                            #   rocprofv3 --kernel-trace --stats -d DIR -- python tools/render_probe.py kernel
    python tools/render_probe.py call       # one graph-free Engine.render call end to end (host clock around a device synchronise), same frames
    python tools/render_probe.py numpy      # tests/render_ref.py on the CPU for ONE of those frames at 800 x 800, as context

MATE-8v8-9, 8 environments, 60 steps under the on-device Greedy agents of both teams (tracked markers, perceived cameras, notched fields of view)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from mate_amd.config import read_config  # noqa: E402
from mate_amd.engine import Engine  # noqa: E402

ENVS, SIZES = 8, (800, 200)


def engine():
    eng = Engine(read_config('MATE-8v8-9.yaml'), ENVS, seed=0)
    eng.enable_policies()
    eng.reset()
    for _ in range(60):
        eng.step_greedy(auto_reset=1)
    torch.cuda.synchronize()
    return eng


def main(what):
    eng = engine()
    if what == 'kernel':
        for size in SIZES:
            out = torch.empty((ENVS, size, size, 3), dtype=torch.uint8, device=eng.device)
            for _ in range(12):
                eng.render(size=size, out=out)
        torch.cuda.synchronize()
        print('12 launches per size', SIZES, 'of', ENVS, 'environments: read the kernel statistics')
    elif what == 'call':
        for size in SIZES:
            out = torch.empty((ENVS, size, size, 3), dtype=torch.uint8, device=eng.device)
            for _ in range(5):
                eng.render(size=size, out=out)
            torch.cuda.synchronize()
            times = []
            for _ in range(50):
                t0 = time.perf_counter()
                eng.render(size=size, out=out)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            times = np.array(times) * 1e6
            print(f'Engine.render of {ENVS} environments at {size} x {size}, call + synchronise: median {np.median(times):.1f} us, min {times.min():.1f}, max {times.max():.1f} (50 calls)')
    else:
        import render_ref as R
        scene = R.scene_of_engine(eng, 0, masks=eng.masks)
        t0 = time.perf_counter()
        prims = R.display_list(scene)
        image = R.rasterise(prims, 800)
        print(f'render_ref, one environment at 800 x 800 on the CPU: {time.perf_counter() - t0:.3f} s ({len(prims)} primitives, {int((image != 255).any(axis=-1).sum())} pixels drawn)')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else 'call')
