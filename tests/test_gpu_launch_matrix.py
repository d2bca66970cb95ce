"""GPU (-m gpu): WHAT EVERY STEPPING ENTRY POINT LAUNCHES (csrc/engine_host.h: plan_step, plan_rollout_random, plan_with_policies).

The 8-environment part of tools/launch_matrix.py -- one list of calls, the tool's -- against tests/golden/launch_flows.json, which holds, per call,
the flow the launch ran (Engine.last_flow), the environments per wave the Greedy rollouts run with (Engine.sub_wave) and the error code of a
call the engine rejects, and per shape what mate_engine_set_sub_wave answers, all recorded at the commit in front of the launch plans (7e507f2).
Each call is also held to the same bits with one and with the shape's number of environments per wave, and no planned launch may fail for want
of an LDS opt-in (policy_enable opts in what the planner can return)."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import launch_matrix as M  # noqa: E402

pytestmark = pytest.mark.gpu

MATE_EHIP = -2      # include/mate_engine.h
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'launch_flows.json')) as fh:
    GOLDEN = json.load(fh)


def same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def compare(what, one, out_one, sub, out_sub):
    """Behind each call: the outputs, both mask buffers and the records of set_sub_wave(False) and set_sub_wave(True), bit for bit."""
    assert (out_one is None) == (out_sub is None), what
    for x, y in zip(out_one or (), out_sub or ()):
        assert same(x, y), what
    assert same(one.masks, sub.masks) and same(one._rollout['masks'], sub._rollout['masks']), what
    assert same(one.export_state(), sub.export_state()), what


def check_columns(record, golden):
    assert sorted(record) == sorted(golden)
    for column, rows in record.items():
        for (name, k), values, want in zip(M.CALL_LIST, rows, golden[column]):
            assert values[2] != MATE_EHIP, (column, name, k)              # (a launch HIP refused: e.g. dynamic LDS nobody opted in to)
            assert values == want, (column, name, k, values, want)
        assert len(rows) == len(golden[column]) == len(M.CALL_LIST)


@pytest.mark.parametrize('shape', M.SHAPES)
def test_every_call_runs_the_flow_recorded_in_front_of_the_launch_plans(shape):
    check_columns(M.small_batch_record(shape, compare), GOLDEN['flows'][shape])


@pytest.mark.parametrize('switch', M.SWITCH_COLUMNS)
def test_the_environment_switches_choose_the_recorded_flows(switch, monkeypatch):
    monkeypatch.setenv(*switch.split('='))        # (read by mate_engine_create)
    check_columns(M.small_batch_record('MATE-2v4-0', compare), GOLDEN['switches'][switch])


def test_set_sub_wave_reports_what_it_reported_in_front_of_the_launch_plans():
    """in_use is plan_with_policies(e, false, -1).E now: the number of the fused Greedy rollouts, LDS fit included."""
    same_device = M.threshold_batch() == GOLDEN['threshold_batch']      # (32 environments per compute unit of the device recorded on)
    for shape in M.IN_USE_SHAPES:
        record, want = M.in_use_record(shape), GOLDEN['in_use'][shape]
        assert record['small'] == want['small'] and (not same_device or record['threshold'] == want['threshold']), (shape, record, want)
