"""The Heuristic target opponent (mate_engine_set_target_opponent), the parts that need no GPU: the NumPy restatement of the drift
(tests/heuristic_ref.py) against the recorded reference on every step of the three heuristic_*.npz fixtures, the census of what those
fixtures exercise, and the argument rules of the Python surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import golden_util as G
from heuristic_ref import fixture_inputs, heuristic_drift

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ['heuristic_4v8-9_s51', 'heuristic_8v8-9_s52', 'heuristic_4v2-9_s53']


@pytest.fixture(scope='module', params=FIXTURES)
def recorded(request):
    fx = G.load(request.param + '.npz')
    final, info = heuristic_drift(**fixture_inputs(fx))
    return request.param, fx, final, info


def test_restatement_reproduces_the_recorded_final_actions(recorded):
    name, fx, final, info = recorded
    assert final.shape == fx['step/tgt_act'].shape and 100 <= len(final) <= 200
    worst = np.abs(final - fx['step/tgt_act']).max()
    print(name, 'worst |restatement - recorded|', worst)
    assert worst < 1e-9, (name, worst)
    # where no camera is a candidate the reference returns the Greedy action itself
    untouched = ~(info['drifted'])
    assert np.array_equal(fx['step/tgt_act'][untouched], fx['step/tgt_act_greedy'][untouched])


def test_fixture_census(recorded):
    name, fx, final, info = recorded
    drifted, rejected = info['drifted'].mean(), info['rejected'].mean()
    print(name, 'drifted', drifted, 'rejected', rejected, 'clipped', int(info['clipped'].sum()), 'multi', int((info['candidates'] >= 2).sum()))
    assert drifted >= 0.20, (name, drifted)
    assert rejected >= 0.02, (name, rejected)
    assert info['clipped'].any(), name
    if '8v8-9' in name:
        assert (info['candidates'] >= 2).any(), name      # the minimum rule is exercised
    # the signed angle test (heuristic.py:308-311): some candidate lies beyond 1.2 half angles on the clockwise side
    kw = fixture_inputs(fx)
    direction = kw['tgt_xy'][:, :, None, :] - kw['cam_xy'][:, None, :, :]
    diff = (np.degrees(np.arctan2(direction[..., 1], direction[..., 0])) - kw['cam_phi'][:, None, :] + 180.0) % 360.0 - 180.0
    in_range = kw['sensed'] & (np.hypot(direction[..., 0], direction[..., 1]) <= 1.2 * kw['cam_sight'][:, None, :])
    assert (in_range & (diff < -1.2 * kw['cam_theta'][:, None, :] / 2.0)).any(), name


def test_no_branch_condition_near_equality(recorded):
    name, fx, final, info = recorded
    margin = info['margin'].min()
    print(name, 'smallest relative branch margin', margin)
    assert margin > 1e-9, (name, margin)


def test_argument_rules_without_a_gpu():
    from mate_amd.config import read_config
    from mate_amd.environment import BatchedMultiAgentTracking, MultiAgentTracking, fragment_arguments
    from mate_amd.engine import Engine, Stepper, TARGET_AGENTS
    assert TARGET_AGENTS == ('greedy', 'heuristic')
    cfg = read_config('MATE-4v8-9.yaml')
    # the fused K-frame launch of a camera learner holds the Greedy agents
    with pytest.raises(AssertionError, match='heuristic'):
        fragment_arguments(cfg, 4, 'camera', target_agent='heuristic')
    with pytest.raises(AssertionError, match='heuristic'):
        BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=4, frame_skip=4, learner='camera', target_agent='heuristic')
    with pytest.raises(AssertionError, match='target_agent'):
        fragment_arguments(cfg, None, None, target_agent='smart')
    with pytest.raises(AssertionError, match='target_agent'):
        BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=4, target_agent='smart')
    # a target learner plays the targets itself: the opponent does not matter there; Greedy stays what it was
    assert fragment_arguments(cfg, 4, 'target', target_agent='heuristic')['learner'] == 'target'
    assert fragment_arguments(cfg, 4, 'camera')['learner'] == 'camera'
    # the opponents' `sensed` is the plain view
    for kw in ({'enhanced_observation': 'target'}, {'shared_field_of_view': 'both'}):
        with pytest.raises(AssertionError, match='plain rows'):
            BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=4, target_agent='heuristic', **kw)
    assert inspect.signature(BatchedMultiAgentTracking.__init__).parameters['target_agent'].default == 'greedy'
    assert inspect.signature(MultiAgentTracking.enable_greedy_policies).parameters['target_agent'].default == 'greedy'
    assert inspect.signature(Engine.enable_policies).parameters['target_agent'].default == 'greedy'
    assert inspect.signature(Engine.policy_actions).parameters['greedy_targets'].default is False
    assert callable(Engine.set_target_opponent) and Stepper is not None


def test_library_header_and_binding_agree():
    from mate_amd import _native
    assert os.path.exists(_native.LIB_PATH), 'run __graft_entry__.build() first'
    lib = ctypes.CDLL(_native.LIB_PATH)
    with open(os.path.join(ROOT, 'include', 'mate_engine.h')) as fh:
        header = fh.read()
    for name in ('mate_engine_set_target_opponent', 'mate_engine_policy_greedy_target_actions'):
        assert hasattr(lib, name) and name in _native.EXPORTED_SYMBOLS, name
        assert re.search(r'int\s+' + name + r'\s*\(', header), name
    assert re.search(r'MATE_OPPONENT_GREEDY\s*=\s*0\s*,\s*MATE_OPPONENT_HEURISTIC\s*=\s*1', header)
    assert '#define MATE_ABI_VERSION 1' in header                      # additive: the ABI number stays


@pytest.mark.parametrize('argv,expected', [(['--target-agent', 'heuristic'], 'heuristic'), ([], 'greedy')])
def test_evaluate_forwards_the_target_agent(monkeypatch, argv, expected):
    """python -m mate_amd.evaluate --target-agent X: the choice reaches enable_greedy_policies (a stand-in environment records the
    call and ends the run there); an unknown agent is refused by the parser."""
    import mate_amd
    import mate_amd.evaluate as E
    calls = []

    class Stop(Exception):
        pass

    class Env:
        def __init__(self, config, **overrides):
            calls.append(('make', config))

        def enable_greedy_policies(self, **kwargs):
            calls.append(('enable', kwargs))

        def seed(self, seed):
            raise Stop

    monkeypatch.setattr(mate_amd, 'MultiAgentTracking', Env)
    monkeypatch.setattr('sys.argv', ['evaluate', '--config', 'MATE-4v2-9.yaml'] + argv)
    with pytest.raises(Stop):
        E.main()
    assert calls == [('make', 'MATE-4v2-9.yaml'), ('enable', {'target_agent': expected})]
    monkeypatch.setattr('sys.argv', ['evaluate', '--target-agent', 'smart'])
    with pytest.raises(SystemExit):
        E.main()
