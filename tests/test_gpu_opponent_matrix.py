"""GPU (-m gpu): WHO PLAYS EACH TEAM OF A CALL, WHICH LAUNCHES THAT TAKES AND WHOSE ROWS THE STEP CONSUMES (csrc/engine_host.h: plan_opponents).

The opponents column set of tools/launch_matrix.py -- one engine per shape, reconfigured through the plain selections, the mixtures and the channels
the setters can reach, every per-step and fused call with the on-device agents under each, and the setters' refusals in both orders of their two
calls -- against tests/golden/opponent_flows.json, which holds per call the error code, the full error text, the flow (Engine.last_flow), which
buffer policy_actions() equals bit for bit and whether the channel edges changed, all recorded (launch_matrix.py opponents --golden) on the build of the
commit in front of the opponent plan (34293a1)."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import launch_matrix as M  # noqa: E402

pytestmark = pytest.mark.gpu

MATE_EHIP = -2      # include/mate_engine.h
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'opponent_flows.json')) as fh:
    GOLDEN = json.load(fh)


def check_row(where, row, want):
    want = GOLDEN['rows'][want]      # (each distinct row once in the file)
    assert row[0] != MATE_EHIP, (where, row[1])      # (a launch HIP refused)
    assert row == want, (where, row, want)


@pytest.mark.parametrize('shape', M.OPPONENT_SHAPES)
def test_every_state_decides_what_it_decided_in_front_of_the_opponent_plan(shape):
    record, golden = M.interned(M.opponents_record(shape), GOLDEN['texts']), GOLDEN['shapes'][shape]      # (each error text once in the file: '#<index>')
    assert list(record['states']) == list(golden['states']) and sorted(record['refusals']) == sorted(golden['refusals'])
    for label, state in record['states'].items():
        assert state['setters'] == golden['states'][label]['setters'], (shape, label)
        column = GOLDEN['columns'][golden['states'][label]['calls']]      # (each distinct list of a state's rows once in the file)
        assert len(state['calls']) == len(column) == len(M.OPPONENT_CALLS)
        for (name, k), row, want in zip(M.OPPONENT_CALLS, state['calls'], column):
            check_row((shape, label, name, k), row, want)
    for what, scenario in record['refusals'].items():
        assert scenario['setters'] == golden['refusals'][what]['setters'], (shape, what)
        check_row((shape, what), scenario['step_greedy'], golden['refusals'][what]['step_greedy'])

