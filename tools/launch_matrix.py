#!/usr/bin/env python3
"""A profiling target: every stepping entry point in every launch form the host can plan (csrc/engine_host.h: plan_step,
plan_rollout_random, plan_with_policies), as one fixed list of calls.  One line per call: the flow the launch ran (Engine.last_flow) and
the environments per wave the Greedy rollouts run with (Engine.sub_wave), or the engine's error code where the call is rejected.
python tools/launch_matrix.py [<shape> [<batch>]]      (default: every shape at both batches)
Under `rocprofv3 --kernel-trace -- python tools/launch_matrix.py ...` the ordered (kernel, grid, workgroup, LDS) list of two builds of
the library (MATE_ENGINE_LIB) must be the same; tests/test_gpu_launch_matrix.py runs the 8-environment part against recorded values.
The environment switches are read when an engine is created: a column under one of SWITCH_COLUMNS is run with the variable set."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, 'tests')):
    if path not in sys.path:
        sys.path.insert(0, path)
from mate_amd._native import EngineError  # noqa: E402
from mate_amd.config import read_config  # noqa: E402
from mate_amd.engine import Engine  # noqa: E402

# E = 4 everywhere | the random flow stays one per wave in auto mode | E = 2, Greedy flows only | row image, E = 1 | generic kernels (tests/shape_edges.py)
SHAPES = ('MATE-2v4-0', 'MATE-4v4-9', 'MATE-4v8-0', 'MATE-4v8-9', '3v5-7')
# every shape with sub-wave kernels (engine_kernels.hpp sub_wave_of: at most four cameras and four targets, and MATE-4v8-0) + the rest of SHAPES
IN_USE_SHAPES = tuple('MATE-%s-%d' % (s, o) for s in ('1v1', '1v2', '2v2', '2v4', '4v2', '4v4') for o in (0, 9)) + ('MATE-4v8-0', 'MATE-4v8-9', '3v5-7')
SMALL_BATCH = 8                      # split-kernel territory; the auto threshold: 32 environments per compute unit (threshold_batch)
DTYPES = ('f32', 'f64')
MODES = (False, True, 'auto')        # Engine.set_sub_wave
AUTO_RESETS = (0, 1, 3)
ROLLOUT_STEPS = 3
CALLS = ('step', 'step_random', 'rollout_random', 'step_greedy', 'step_greedy_tape', 'step_versus_greedy_camera', 'step_versus_greedy_target',
         'rollout_greedy', 'rollout_versus_greedy_camera', 'rollout_versus_greedy_target')
CALL_LIST = [('observe', 0)] + [(name, k) for name in CALLS for k in AUTO_RESETS]
# the small-batch MATE-2v4-0 column again under each of these (read at create)
SWITCH_COLUMNS = ('MATE_STEP_SUBWAVE=0', 'MATE_STEP_GREEDY_ROLLOUT=1', 'MATE_POLICY_SPLIT=1', 'MATE_STEP_SPLIT=0', 'MATE_STEP_SPLIT=1')


def threshold_batch():
    return 32 * torch.cuda.get_device_properties(0).multi_processor_count


def config_of(shape):
    if shape.startswith('MATE-'):
        return read_config(shape + '.yaml', max_episode_steps=7)
    import shape_edges
    nc, rest = shape.split('v')
    nt, no = rest.split('-')
    return read_config(dict(shape_edges.scenario((int(nc), int(nt), int(no))), max_episode_steps=7))


def make_engine(shape, batch, dtype, transform, mode):
    """(engine, in_use): policies on, reset, rollout buffers reserved; `in_use`: what set_sub_wave(mode) answered."""
    eng = Engine(config_of(shape), batch, seed=11, first_env_index=2, obs_dtype=torch.float64 if dtype == 'f64' else torch.float32)
    in_use = eng.set_sub_wave(mode)
    eng.enable_policies()
    if transform:
        eng.set_obs_transform(relative_coordinates=True)
    eng.reset()
    eng.reserve_rollout(ROLLOUT_STEPS, want_masks=True, search='none')
    return eng, in_use


def actions_of(eng):
    gen = torch.Generator().manual_seed(7)
    cam = ((torch.rand((eng.num_envs, eng.num_cameras, 2), generator=gen) * 2 - 1) * torch.tensor([5.0, 2.5])).to(eng.device)
    tgt = ((torch.rand((eng.num_envs, eng.num_targets, 2), generator=gen) * 2 - 1) * 20.0).to(eng.device)
    tape = {'target_choice_u': torch.full((eng.num_envs, eng.num_targets), 0.5, dtype=torch.float64, device=eng.device)}
    return cam, tgt, tape


def issue(eng, name, k, acts):
    """One call of CALL_LIST; returns the tensors it wrote."""
    cam, tgt, tape = acts
    if name == 'observe':
        return eng.observe()
    if name == 'step':
        return eng.step(cam, tgt, auto_reset=k)
    if name == 'step_random':
        return eng.step_random(auto_reset=k, want_masks=True)
    if name == 'rollout_random':
        return eng.rollout_random(ROLLOUT_STEPS, auto_reset=k, want_masks=True)
    if name == 'step_greedy':
        return eng.step_greedy(auto_reset=k)
    if name == 'step_greedy_tape':
        return eng.step_greedy(policy_tape=tape, auto_reset=k)
    if name == 'rollout_greedy':
        return eng.rollout_greedy(ROLLOUT_STEPS, auto_reset=k, want_masks=True)
    kind, team = name.rsplit('_', 1)
    mine = cam if team == 'camera' else tgt
    if kind == 'step_versus_greedy':
        return eng.step_versus_greedy(team, mine, auto_reset=k)
    assert kind == 'rollout_versus_greedy', name
    return eng.rollout_versus_greedy(team, mine, ROLLOUT_STEPS, auto_reset=k, want_masks=True)


def run_column(eng):
    """Issues CALL_LIST on `eng`; yields (call id, [last_flow, sub_wave, error code], outputs or None) behind each call."""
    acts = actions_of(eng)
    for name, k in CALL_LIST:
        code, out = 0, None
        try:
            out = issue(eng, name, k, acts)
        except EngineError as err:
            code = err.code
        yield '%s/%d' % (name, k), [eng.last_flow, eng.sub_wave, code], out


def column_id(shape, dtype, transform, mode):
    return '%s %s %s sub_wave=%s' % (shape, dtype, 'transform' if transform else 'plain', mode)


def small_batch_record(shape, compare=None):
    """{column id: [[last_flow, sub_wave, error code] of every call of CALL_LIST]}: the 8-environment columns of `shape`, the three modes of
    a column stepped side by side.  compare(what, engine of set_sub_wave(False), its outputs, engine of (True), its outputs) behind each call."""
    record = {}
    for dtype in DTYPES:
        for transform in (False, True):
            engines = [make_engine(shape, SMALL_BATCH, dtype, transform, mode)[0] for mode in MODES]
            rows = [[] for _ in MODES]
            for results in zip(*[run_column(eng) for eng in engines]):
                for row, (_, values, _) in zip(rows, results):
                    row.append(values)
                if compare:
                    compare('%s %s' % (column_id(shape, dtype, transform, 'False/True'), results[0][0]), engines[0], results[0][2], engines[1], results[1][2])
            torch.cuda.synchronize()
            for mode, row, eng in zip(MODES, rows, engines):
                record[column_id(shape, dtype, transform, mode)] = row
                eng.close()
    return record


def in_use_record(shape):
    """{'small' | 'threshold': [set_sub_wave(mode) for the three modes, ahead of enable_policies() | behind it]}"""
    record = {}
    for label, batch in (('small', SMALL_BATCH), ('threshold', threshold_batch())):
        eng = Engine(config_of(shape), batch, seed=11)
        before = [eng.set_sub_wave(mode) for mode in MODES]
        eng.enable_policies()
        record[label] = [before, [eng.set_sub_wave(mode) for mode in MODES]]
        eng.close()
    return record


def main(argv):
    shapes = argv[1:2] or SHAPES
    batches = [int(argv[2])] if len(argv) > 2 else [SMALL_BATCH, threshold_batch()]
    calls = 0
    for shape in shapes:
        for batch in batches:
            for dtype in DTYPES:
                for transform in (False, True):
                    for mode in MODES:
                        eng, in_use = make_engine(shape, batch, dtype, transform, mode)
                        print(column_id(shape, dtype, transform, mode), 'batch', batch, 'in_use', in_use, flush=True)
                        for call, values, _ in run_column(eng):
                            print('  %-32s flow %d sub_wave %d error %d' % (call, *values))
                            calls += 1
                        torch.cuda.synchronize()
                        eng.close()
    print('done', calls, 'calls')


if __name__ == '__main__':
    main(sys.argv)
