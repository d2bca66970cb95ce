#!/usr/bin/env python3
"""Cost of FrameSkip fragments on the fused K-frame launch (Engine.enable_fragment_rows): µs per graph-replayed
fragment of
  (a) rollout_versus_greedy + the torch reduction (live mask, arg-max of the last live frame, gather, column transform, column sums,
      means, last-frame info; with shaping the coverage_rate sum) -- the only way before the fragment launch; it calls engine entry
      points that predate the launch only, its outputs are its own tensors and its column table is host-side NumPy (mate_amd.spaces),
  (b) rollout_versus_greedy + the attached fragment launch,
  (c) K x step_versus_greedy with the packer's fused transform and accumulating reward rows -- the only way to shaped FrameSkip before,
  (d) (b) with the first rows of restarted episodes on (enable_fragment_rows(first_rows=True, final_obs=True)): one memset node and two
      one-frame launches of the fragment kernel more per fragment; (d) - (b) is the feature's cost, (b) itself is the feature off,
on MATE-4v8-9 (camera learner, {'coverage_rate': 1.0} 'mean', K = 5) and MATE-2v4-0 (target learner, unshaped, K = 10), each at 4096 and
16 384 environments, all four in one process, interleaved; `--series` repeated series of `--rounds` timed blocks give the run-to-run
spread next to the medians.  Prints the table; `--out` also writes it (profiles/fragment_probe.txt).

    python tools/fragment_probe.py --out profiles/fragment_probe.txt
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
from mate_amd.spaces import fragment_column_table  # noqa: E402

LEGS = 'abcd'
WORKLOADS = (('MATE-4v8-9.yaml', 'camera', 5, ({'coverage_rate': 1.0}, 'mean')), ('MATE-2v4-0.yaml', 'target', 10, None))


def torch_fragment(eng, team, K, table, shaped, out):
    """FrameSkip's reduction over the rollout-shaped buffers in torch (what a caller of the fused launch had to write)."""
    buf = eng.reserve_rollout(K)
    rows, sc = (buf['camera_obs'] if team == 'camera' else buf['target_obs'])[:K], buf['scalars'][:K]
    n = eng.num_envs
    sub, flag, scale, bias = (torch.as_tensor(t, device=eng.device) for t in table)
    scale, bias = scale.to(rows.dtype), bias.to(rows.dtype)
    own_index = torch.tensor([0, 13, 14], device=eng.device)[sub.long()]
    gate_index = flag.clamp(min=0).long()
    env = torch.arange(n, device=eng.device)
    frames = torch.arange(K, device=eng.device)[:, None]
    # every index lives on the device before the capture: a Python list index would be uploaded at every call
    team_columns, rate_columns, last_columns = (torch.tensor(c, device=eng.device) for c in ([0, 1, 7], [3, 4], [5, 6]))

    def between():
        live = sc[..., 2] != 2
        s = torch.where(live[..., None], sc, torch.zeros_like(sc)).double()
        count = live.sum(0)
        last = torch.where(live, frames, torch.full_like(frames, -1)).amax(0).clamp(min=0)
        picked = rows[last, env]
        own = torch.where(sub != 0, picked[..., own_index], torch.zeros_like(picked))
        visible = (flag < 0) | (picked[..., gate_index] != 0)
        out['obs'].copy_(torch.where(visible, picked - own, torch.zeros_like(picked)) * scale + bias)
        sums = s.index_select(-1, team_columns).sum(0)
        out['rewards'][:, :3] = sums
        out['rewards'][:, 3] = -sums[:, 2]
        out['done'].copy_(((sc[..., 2] == 1) & live).any(0))
        out['frames'].copy_(count)
        out['info'][:, :2] = s.index_select(-1, rate_columns).sum(0) / count.clamp(min=1)[:, None]
        out['info'][:, 2:] = sc[last, env].index_select(-1, last_columns).double()
        if shaped:
            out['shaped'].copy_(s[..., 3].sum(0)[:, None].expand_as(out['shaped']))
    return between


def build(kind, cfg, n, team, K, shaping):
    eng = Engine(cfg, n, seed=1)
    if kind == 'c':
        eng.set_obs_transform(True, True)
    eng.enable_policies()
    eng.reset()
    agents = eng.num_cameras if team == 'camera' else eng.num_targets
    act = torch.zeros((n, agents, 2), dtype=torch.float64, device=eng.device)
    acts = (act, None) if team == 'camera' else (None, act)
    if kind == 'c':
        if shaping is not None:
            eng.enable_reward_rows(**{team: shaping}, accumulate=True)
        return eng, eng.make_stepper(*acts, auto_reset=K, graph_steps=2 * K, versus=team), K
    between = None
    if kind in 'bd':
        eng.enable_fragment_rows(team, K, shaping=shaping, relative_coordinates=True, rescaled_observation=True, first_rows=kind == 'd', final_obs=kind == 'd')
    if kind == 'a':
        table = fragment_column_table(team, eng.num_cameras, eng.num_targets, eng.num_obstacles, True, True)
        D = eng.camera_obs_dim if team == 'camera' else eng.target_obs_dim
        new = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=eng.device)  # noqa: E731
        out = {'obs': new((n, agents, D), eng.obs_dtype), 'rewards': new((n, 4), torch.float64), 'info': new((n, 4), torch.float64),
               'done': new(n, torch.bool), 'frames': new(n, torch.int32), 'shaped': new((n, agents), torch.float64)}
        eng.reserve_rollout(K)
        between = torch_fragment(eng, team, K, table, shaping is not None, out)
        # the reduction FOLLOWS the launch: the stepper's `between` runs ahead of it, so it reduces the previous fragment -- the same work per fragment
    stepper = eng.make_stepper(*acts, auto_reset=True, graph_steps=2, between=between, versus=team, frame_skip=K)
    return eng, stepper, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--series', type=int, default=3)
    ap.add_argument('--fragments', type=int, default=200, help='fragments per timed block')
    ap.add_argument('--out')
    args = ap.parse_args()
    lines = ['graph-replayed, us per fragment: median over %d series x %d blocks of %d fragments [min .. max of the series medians]' % (args.series, args.rounds, args.fragments),
             '| scenario | learner | K | envs | (a) fused + torch reduction | (b) fused + fragment launch | (c) K per-step launches | (d) (b) + first rows | (a) - (b) | (c) / (b) | (d) - (b) |', '|---|---|---|---|---|---|---|---|---|---|---|']
    for config, team, K, shaping in WORKLOADS:
        cfg = read_config(config)
        for n in (4096, 16384):
            flows = {kind: build(kind, cfg, n, team, K, shaping) for kind in LEGS}
            for eng, stepper, per in flows.values():
                stepper.run(args.fragments * per)      # warm-up
            torch.cuda.synchronize()
            medians = {kind: [] for kind in LEGS}
            for _ in range(args.series):
                times = {kind: [] for kind in LEGS}
                for _ in range(args.rounds):
                    for kind, (eng, stepper, per) in flows.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        stepper.run(args.fragments * per)
                        torch.cuda.synchronize()
                        times[kind].append((time.perf_counter() - t0) / args.fragments * 1e6)
                for kind in LEGS:
                    medians[kind].append(statistics.median(times[kind]))
            med = {kind: statistics.median(v) for kind, v in medians.items()}
            cell = lambda kind: '%.2f [%.2f .. %.2f]' % (med[kind], min(medians[kind]), max(medians[kind]))  # noqa: E731
            lines.append('| %s | %s | %d | %d | %s | %s | %s | %s | %.2f | %.2f | %.2f |' % (config[:-5], team, K, n, cell('a'), cell('b'), cell('c'), cell('d'), med['a'] - med['b'], med['c'] / med['b'],
                                                                                      med['d'] - med['b']))
            for eng, stepper, per in flows.values():
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
