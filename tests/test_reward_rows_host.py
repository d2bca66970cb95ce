"""Host side of the shaped reward rows (no GPU): the coefficient tables' order, the shapers' assertions, the C header and its binding.
(The kernels' register / scratch figures: tests/test_kernel_resources.py.)"""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_coefficient_tables_follow_the_key_tuples():
    from mate_amd.auxiliary_rewards import AuxiliaryTargetRewards
    from mate_amd.engine import REWARD_REDUCTIONS, reward_coefficient_table, reward_term_keys
    from mate_amd.environment import BatchedMultiAgentTracking
    assert reward_term_keys('camera') == BatchedMultiAgentTracking.AUXILIARY_REWARD_KEYS and len(reward_term_keys('camera')) == 7
    assert reward_term_keys('target') == AuxiliaryTargetRewards.ACCEPTABLE_KEYS and len(reward_term_keys('target')) == 10
    for team in ('camera', 'target'):
        keys = reward_term_keys(team)
        for k, key in enumerate(keys):                       # one key at a time lands in its own slot
            table, reduction = reward_coefficient_table(team, {key: k + 1.5}, 'sum')
            assert table == [k + 1.5 if i == k else 0.0 for i in range(len(keys))] and reduction == REWARD_REDUCTIONS['sum'] == 2
        everything = {key: float(i + 1) for i, key in reversed(list(enumerate(keys)))}      # the mapping's own order does not matter
        assert reward_coefficient_table(team, everything)[0] == [float(i + 1) for i in range(len(keys))]
    assert REWARD_REDUCTIONS == {'none': 0, 'mean': 1, 'sum': 2, 'max': 3, 'min': 4}


def test_key_and_reduction_assertions_carry_the_references_messages():
    from mate_amd.engine import reward_coefficient_table
    with pytest.raises(AssertionError, match=r'The coefficient mapping only accepts keys in \(.*\)\. Got list\(coefficients\.keys\(\)\) = \[\'is_tracked\'\]\.'):
        reward_coefficient_table('camera', {'is_tracked': 1.0})             # a target term
    with pytest.raises(AssertionError, match=r'The coefficient mapping only accepts keys in'):
        reward_coefficient_table('target', {'num_tracked': 1.0})            # a camera term
    with pytest.raises(AssertionError, match=r'Invalid reduction method median\.'):
        reward_coefficient_table('camera', {'baseline': 1.0}, 'median')
    with pytest.raises(AssertionError, match=r'Invalid reduction method min\. The reduction method should be one of'):
        reward_coefficient_table('target', {'baseline': 1.0}, 'min')        # the camera wrapper's alone
    with pytest.raises(AssertionError, match='only constant coefficients'):
        reward_coefficient_table('target', {'baseline': lambda *args: 1.0})
    assert reward_coefficient_table('camera', {'baseline': 1}, 'min')[1] == 4


def test_header_declares_the_entry_point_and_the_binding_matches():
    from mate_amd import _native
    with open(os.path.join(ROOT, 'include', 'mate_engine.h')) as fh:
        header = fh.read()
    assert '#define MATE_ABI_VERSION 1' in header
    for symbol in ('mate_engine_enable_reward_rows', 'typedef struct mate_reward_rows', 'MATE_REDUCE_NONE = 0', 'MATE_REDUCE_MIN = 4',
                   'MATE_CAMERA_REWARD_TERMS 7', 'MATE_TARGET_REWARD_TERMS 10'):
        assert symbol in header, symbol
    declaration = re.search(r'int mate_engine_enable_reward_rows\(([^)]*)\);', header).group(1)
    assert len(declaration.split(',')) == 2
    assert 'mate_engine_enable_reward_rows' in _native.EXPORTED_SYMBOLS
    # the struct's members, in the header's order, are the binding's fields
    body = re.search(r'typedef struct mate_reward_rows \{(.*?)\} mate_reward_rows;', header, re.S).group(1)
    members = re.findall(r'(\w+)\s*[,;]', body)
    assert members == [name for name, _ in _native.MateRewardRows._fields_], members
    assert ctypes.sizeof(_native.MateRewardRows) == 4 * 8 + 5 * 4 + 4 + 2 * 8      # four pointers, five ints (+ padding), two pointers
    if os.path.exists(_native.LIB_PATH):      # (built: the symbol resolves and takes two arguments)
        handle = _native.load()
        assert len(handle.mate_engine_enable_reward_rows.argtypes) == 2
        assert handle.mate_engine_enable_reward_rows(None, None) == -1         # MATE_EINVAL: null engine
