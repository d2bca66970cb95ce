"""CPU-only tests of the Python host's three rules (host section): the C ABI is bound from one prototype table that agrees
with include/mate_engine.h, the scenario mapping is turned into the engine's tables in one function, and every attribute an Engine, a
Stepper or a BatchedMultiAgentTracking can hold is declared in its __init__."""
import ast
import inspect
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def header():
    with open(os.path.join(ROOT, 'include', 'mate_engine.h')) as fh:
        return re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)      # (comments name functions and use parentheses too)


def test_prototype_table_has_the_arity_of_every_declaration(header):
    from mate_amd import _native
    declared = re.findall(r'\b(mate_engine_[a-z_]+)\s*\(([^()]*)\)\s*;', header)
    assert len(declared) == len({name for name, _ in declared}) >= 57
    assert {name for name, _ in declared} == set(_native.PROTOTYPES) == set(_native.EXPORTED_SYMBOLS)
    for name, params in declared:
        count = 0 if params.strip() == 'void' else len(params.split(','))
        restype, argtypes = _native.PROTOTYPES[name]
        assert len(argtypes) == count, (name, params)
    lib = _native.load()
    for name, (restype, argtypes) in _native.PROTOTYPES.items():      # load() applied the table
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == list(argtypes), name


def test_structures_have_the_members_of_the_header_in_order(header):
    from mate_amd import _native
    structures = {'mate_config': _native.MateConfig, 'mate_layout': _native.MateLayout, 'mate_step_io': _native.MateStepIO,
                  'mate_policy_tape': _native.MatePolicyTape, 'mate_reward_rows': _native.MateRewardRows,
                  'mate_fragment_rows': _native.MateFragmentRows, 'mate_first_rows': _native.MateFirstRows}
    bodies = dict(re.findall(r'typedef\s+struct\s+(mate_\w+)\s*\{(.*?)\}\s*\1\s*;', header, flags=re.S))
    assert set(bodies) == set(structures)
    for name, body in bodies.items():
        members = []
        for declaration in filter(None, (d.strip() for d in body.split(';'))):
            for declarator in declaration.split(','):      # "int32_t a, b", "const double *p", "double r[2]"
                members.append(re.search(r'(\w+)\s*(\[\d+\])?$', declarator.strip()).group(1))
        assert members == [field[0] for field in structures[name]._fields_], name


def test_scenario_tables_of_every_branch():
    from mate_amd.config import read_config, scenario_tables

    def rows(a):
        return np.asarray(a, dtype=np.float64).tolist()

    # fixed `location` only (the cameras of MATE-2v2-0), no obstacle section at all
    t = scenario_tables(read_config('MATE-2v2-0.yaml'))
    assert (t['num_cameras'], t['num_targets'], t['num_obstacles']) == (2, 2, 0)
    assert rows(t['camera_ranges']) == [[-300.0, -300.0, -300.0, -300.0], [300.0, 300.0, 300.0, 300.0]]
    assert rows(t['target_ranges']) == [[-200.0, 200.0, -200.0, 200.0]] * 2
    assert t['obstacle_ranges'].shape == (0, 4) and t['obstacle_radius_range'] == (0.0, 0.0) and t['transmittance'] == 0.0
    assert t['camera'] == {'radius': 40.0, 'min_viewing_angle': 30.0, 'max_sight_range': 1500.0, 'rotation_step': 5.0, 'zooming_step': 2.5}
    # `location_random_range` only, `radius_random_range` (MATE-4v2-9)
    t = scenario_tables(read_config('MATE-4v2-9.yaml'))
    assert (t['num_cameras'], t['num_targets'], t['num_obstacles']) == (4, 2, 9)
    assert rows(t['camera_ranges']) == [[500.0, 800.0, 500.0, 800.0], [500.0, 800.0, -800.0, -500.0], [-800.0, -500.0, -800.0, -500.0],
                                        [-800.0, -500.0, 500.0, 800.0]]
    assert rows(t['obstacle_ranges'])[4] == [900.0, 900.0, -500.0, 500.0] and rows(t['obstacle_ranges'])[8] == [-200.0, 200.0, -200.0, 200.0]
    assert t['obstacle_radius_range'] == (25.0, 100.0) and t['transmittance'] == 0.1
    # both: the fixed sites come first; a fixed obstacle `radius` is the degenerate range
    t = scenario_tables(read_config('MATE-2v2-0.yaml', camera={'location_random_range': [[500, 800, -800, -500]], 'radius': 25},
                                    obstacle={'location': [[0.0, 100.0]], 'radius': 30}))
    assert rows(t['camera_ranges']) == [[-300.0, -300.0, -300.0, -300.0], [300.0, 300.0, 300.0, 300.0], [500.0, 800.0, -800.0, -500.0]]
    assert rows(t['obstacle_ranges']) == [[0.0, 0.0, 100.0, 100.0]] and t['obstacle_radius_range'] == (30.0, 30.0)
    assert (t['num_cameras'], t['num_obstacles']) == (3, 1) and t['camera']['radius'] == 25.0 and isinstance(t['camera']['radius'], float)
    # no camera section: entities.py's defaults
    t = scenario_tables(read_config('MATE-Navigation.yaml'))
    assert (t['num_cameras'], t['num_targets'], t['num_obstacles']) == (0, 8, 32) and t['camera_ranges'].shape == (0, 4)
    assert t['camera'] == {'radius': 40.0, 'min_viewing_angle': 90.0, 'max_sight_range': 500.0, 'rotation_step': 5.0, 'zooming_step': 2.5}
    assert list(t['camera']) == ['radius', 'min_viewing_angle', 'max_sight_range', 'rotation_step', 'zooming_step']
    assert rows(t['obstacle_ranges'])[:2] == [[200.0, 800.0, 200.0, 800.0], [200.0, 800.0, -800.0, -200.0]]
    # a scenario of its own through overrides: the 2v3-64 trace fixture's
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'trace_2v3-64_random_s8.npz')) as fx:
        config = read_config(str(fx['config_file']), **json.loads(str(fx['overrides'])))
    t = scenario_tables(config)
    assert (t['num_cameras'], t['num_targets'], t['num_obstacles']) == (2, 3, 64)
    assert rows(t['camera_ranges']) == [[-200.0, -200.0, -200.0, -200.0], [200.0, 200.0, 200.0, 200.0]]
    assert rows(t['target_ranges']) == [[142.0, 258.0, 142.0, 258.0]] * 3
    assert rows(t['obstacle_ranges'])[0] == [-725.0, -675.0, -725.0, -675.0] and rows(t['obstacle_ranges'])[63] == [675.0, 725.0, 675.0, 725.0]
    assert t['obstacle_radius_range'] == (6.0, 16.0) and t['transmittance'] == 0.1 and t['camera']['max_sight_range'] == 1500.0
    for key in ('camera_ranges', 'target_ranges', 'obstacle_ranges'):
        assert t[key].dtype == np.float64 and t[key].flags['C_CONTIGUOUS'] and t[key].shape[1] == 4


def _self_attributes(function, follow=None):
    """Names assigned on `self` inside `function`: plain `self.x = ...` targets (tuples and chains included) and setattr(self, 'literal', ...);
    `follow`: the class's methods by name -- those called as an unconditional `self.method()` statement of the body are included."""
    names = set()
    for node in ast.walk(function):
        targets = node.targets if isinstance(node, ast.Assign) else [node.target] if isinstance(node, (ast.AugAssign, ast.AnnAssign)) else []
        for target in targets:
            for leaf in ast.walk(target):
                if isinstance(leaf, ast.Attribute) and isinstance(leaf.value, ast.Name) and leaf.value.id == 'self' and isinstance(leaf.ctx, ast.Store):
                    names.add(leaf.attr)
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == 'setattr' and len(node.args) == 3 \
                and isinstance(node.args[0], ast.Name) and node.args[0].id == 'self' and isinstance(node.args[1], ast.Constant):
            names.add(node.args[1].value)
    for statement in function.body if follow else ():
        call = statement.value if isinstance(statement, ast.Expr) else None
        if isinstance(call, ast.Call) and isinstance(call.func, ast.Attribute) and isinstance(call.func.value, ast.Name) \
                and call.func.value.id == 'self' and call.func.attr in follow:
            names |= _self_attributes(follow[call.func.attr], follow)
    return names


@pytest.mark.parametrize('module,name', [('engine', 'Engine'), ('engine', 'Stepper'), ('environment', 'BatchedMultiAgentTracking')])
def test_every_attribute_is_declared_in_init(module, name):
    import importlib
    tree = ast.parse(inspect.getsource(importlib.import_module('mate_amd.' + module)))
    cls = next(node for node in tree.body if isinstance(node, ast.ClassDef) and node.name == name)
    methods = {node.name: node for node in cls.body if isinstance(node, ast.FunctionDef)}
    declared = _self_attributes(methods['__init__'], follow=methods)
    assert len(declared) >= 10
    for method in methods.values():
        undeclared = _self_attributes(method) - declared
        assert not undeclared, f'{name}.{method.name} assigns {sorted(undeclared)}: not declared in {name}.__init__'
