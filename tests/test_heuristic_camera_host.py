"""The Heuristic camera opponent (mate_engine_set_camera_opponent), the parts that need no GPU: the NumPy restatement of the controller and
of act() (tests/heuristic_camera_ref.py) against the recorded reference on every step of the three heuristic_camera_*.npz fixtures, the
tables of mate_amd/heuristic_tables.py against the recorded mesh, grid and score rows, and the argument rules of the Python surface
(the new kernel's resource record: tests/test_unit_resources.py)."""
import ctypes
import hashlib
import inspect
import os
import re

import numpy as np
import pytest

import golden_util as G
from heuristic_camera_ref import fixture_inputs, heuristic_cameras, sensed_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ['heuristic_camera_4v8-9_s61', 'heuristic_camera_8v8-9_s62', 'heuristic_camera_2v4-0_s65']


def tables_of(fx):
    from mate_amd.heuristic_tables import heuristic_camera_tables
    return heuristic_camera_tables(float(fx['static/cam_max_sight_range'][0]), float(fx['static/cam_min_viewing_angle'][0]))


@pytest.fixture(scope='module', params=FIXTURES)
def recorded(request):
    fx = G.load(request.param + '.npz')
    action, index, goal, info = heuristic_cameras(tables=tables_of(fx), **fixture_inputs(fx))
    return request.param, fx, action, index, goal, info


def test_restatement_reproduces_the_recorded_goals_and_actions(recorded):
    name, fx, action, index, goal, info = recorded
    assert index.shape == fx['step/hcam_goal_index'].shape and 60 <= len(index) <= 120
    assert np.array_equal(index, fx['step/hcam_goal_index']), name
    assert np.array_equal(np.isnan(goal), np.isnan(fx['step/hcam_goal'])), name
    assert np.array_equal(np.nan_to_num(goal), np.nan_to_num(fx['step/hcam_goal'])), name
    worst = np.abs(action - fx['step/cam_act']).max()
    print(name, 'worst |restatement - recorded action|', worst)
    assert worst < 1e-9, (name, worst)
    perms = fx['step/hcam_permutations']
    assert perms.shape == (len(index), 32, int(fx['num_cameras']))
    assert (np.sort(perms, axis=-1) == np.arange(perms.shape[-1])).all()


def test_no_decision_near_a_tie(recorded):
    name, fx, action, index, goal, info = recorded
    margin = info['margin'].min()
    print(name, 'smallest relative decision margin', margin)
    assert margin > 1e-9, (name, margin)


def test_fixture_census(recorded):
    name, fx, action, index, goal, info = recorded
    none = index < 0
    print(name, 'no goal', none.mean(), 'kept', int(info['kept'].sum()), 'resampled', int(info['resampled'].sum()),
          'picks off the solo argmax', int(info['solo_differs'].sum()))
    assert none.mean() >= 0.05 and info['kept'].any() and info['resampled'].any(), name
    if '8v8-9' in name:
        assert info['solo_differs'].any(), name      # the tracked-bit interaction between cameras is exercised
    # a goal exists exactly where the camera has a sensed target in range, even where the chosen state scores nothing
    assert np.array_equal(~none, info['counts'] > 0)


def test_sensed_order_is_insertion_order():
    seen = np.zeros((3, 5), dtype=bool)
    seen[0, [3, 1]] = True
    seen[1, [0, 3]] = True
    seen[2, [4, 1, 2]] = True
    assert sensed_order(seen) == [1, 3, 0, 2, 4]


def test_tables_against_the_recorded_reference(recorded):
    name, fx = recorded[:2]
    mesh, grid, scores = tables_of(fx)
    assert mesh.shape == (756, 3) and grid.shape == (2952, 2) and scores.shape == (2952, 756) and scores.dtype == np.float64
    assert np.abs(mesh[:, :2] - fx['table/state_mesh'][:, :2]).max() < 1e-12
    assert np.abs(mesh - fx['table/state_mesh']).max() < 1e-12 * float(fx['static/cam_max_sight_range'][0])
    assert np.abs(grid - fx['table/coord_grid']).max() < 1e-12 * float(fx['static/cam_max_sight_range'][0])
    rows = fx['table/score_row_index']
    assert len(rows) == 24
    assert np.abs(scores[rows] - fx['table/score_rows']).max() < 1e-12
    assert np.array_equal(scores[rows] > 0, fx['table/score_rows'] > 0)
    print(name, 'recorded sha256', str(fx['table/scores_sha256']), 'here', hashlib.sha256(scores.tobytes()).hexdigest(),
          'non-zero share', float((scores > 0).mean()))
    assert 0.10 < (scores > 0).mean() < 0.20
    # state s = a * 36 + o, point g = p * 41 + r
    assert mesh[37, 0] == -170.0 and mesh[36, 1] == mesh[37, 1] > mesh[0, 1] and mesh[-1, 1] == 180.0
    assert np.array_equal(grid[0], [0.0, 0.0]) and abs(np.hypot(*grid[40]) - float(fx['static/cam_max_sight_range'][0])) < 1e-9


def test_tables_are_cached_per_rounded_pair():
    from mate_amd.heuristic_tables import heuristic_camera_tables
    a = heuristic_camera_tables(2000.0, 30.0)
    b = heuristic_camera_tables(2000.0 + 1e-10, 30.0 - 1e-10)
    assert all(x is y for x, y in zip(a, b))
    assert not a[2].flags.writeable


def test_argument_rules_without_a_gpu():
    from mate_amd.config import read_config
    from mate_amd.environment import BatchedMultiAgentTracking, MultiAgentTracking, fragment_arguments
    from mate_amd.engine import CAMERA_AGENTS, Engine
    assert CAMERA_AGENTS == ('greedy', 'heuristic')
    cfg = read_config('MATE-4v8-9.yaml')
    # the fused K-frame launch of a target learner holds the Greedy agents
    with pytest.raises(AssertionError, match='heuristic'):
        fragment_arguments(cfg, 4, 'target', camera_agent='heuristic')
    with pytest.raises(AssertionError, match='heuristic'):
        BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=4, frame_skip=4, learner='target', camera_agent='heuristic')
    with pytest.raises(AssertionError, match='camera_agent'):
        fragment_arguments(cfg, None, None, camera_agent='smart')
    with pytest.raises(AssertionError, match='camera_agent'):
        BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=4, camera_agent='smart')
    # a camera learner plays the cameras itself: the opponent does not matter there; Greedy stays what it was
    assert fragment_arguments(cfg, 4, 'camera', camera_agent='heuristic')['learner'] == 'camera'
    assert fragment_arguments(cfg, 4, 'target')['learner'] == 'target'
    for kw in ({'enhanced_observation': 'camera'}, {'shared_field_of_view': 'both'}):
        with pytest.raises(AssertionError, match='plain rows'):
            BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=4, camera_agent='heuristic', **kw)
    assert inspect.signature(BatchedMultiAgentTracking.__init__).parameters['camera_agent'].default == 'greedy'
    assert inspect.signature(MultiAgentTracking.enable_greedy_policies).parameters['camera_agent'].default == 'greedy'
    assert inspect.signature(Engine.enable_policies).parameters['camera_agent'].default == 'greedy'
    assert callable(Engine.set_camera_opponent) and callable(Engine.heuristic_camera_goals) and callable(Engine.heuristic_camera_tape)


def test_library_header_and_binding_agree():
    from mate_amd import _native
    assert os.path.exists(_native.LIB_PATH), 'run __graft_entry__.build() first'
    lib = ctypes.CDLL(_native.LIB_PATH)
    with open(os.path.join(ROOT, 'include', 'mate_engine.h')) as fh:
        header = fh.read()
    for name in ('mate_engine_set_camera_opponent', 'mate_engine_heuristic_camera_tables', 'mate_engine_heuristic_camera_tape',
                 'mate_engine_heuristic_camera_goals'):
        assert hasattr(lib, name) and name in _native.EXPORTED_SYMBOLS, name
        assert re.search(r'int\s+' + name + r'\s*\(', header), name
    assert '#define MATE_ABI_VERSION 1' in header                      # additive: the ABI number stays


@pytest.mark.parametrize('argv,expected', [(['--camera-agent', 'heuristic'], {'target_agent': 'greedy', 'camera_agent': 'heuristic'}),
                                           (['--camera-agent', 'heuristic', '--target-agent', 'heuristic'], {'target_agent': 'heuristic', 'camera_agent': 'heuristic'})])
def test_evaluate_forwards_the_camera_agent(monkeypatch, argv, expected):
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
    assert calls == [('make', 'MATE-4v2-9.yaml'), ('enable', expected)]
    monkeypatch.setattr('sys.argv', ['evaluate', '--camera-agent', 'smart'])
    with pytest.raises(SystemExit):
        E.main()
