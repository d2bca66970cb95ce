"""Host-side tests of mate_amd/central.py, no GPU and no library: the action descriptor, the width of one teammate's entry and
the column map of the centralised-training rows against tests/central_ref.py, over every accepted and refused combination tests/test_central_host.py lists."""
import itertools

import numpy as np
import pytest
import torch

import central_ref as R
from mate_amd import central as C

LAYOUTS = ((4, 145, 153, 2, 0, True), (8, 113, 153, 25, 0, False), (4, 145, 153, 16, 16, True), (1, 20, 43, 2, 0, True), (7, 33, 151, 1, 6, False))      # (test_central_host.py)
REFUSED = (('f32', 2, 2), ('f64', 3, 0), ('index', 2, 0), ('index', 1, 1), ('bits', 0, 0), ('bits', 17, 0), ('bits', 4, 3), ('pair', 2, 0))      # (test_central_host.py)


def _inputs(kind, components, levels):
    """(dtype, shape, keywords) of central.descriptor that spell the reference's descriptor (kind, components, levels)."""
    if kind in ('f32', 'f64'):
        return (torch.float32 if kind == 'f32' else torch.float64), (3, 4, components), dict(onehot=levels != 0, levels=levels)
    if kind == 'index':
        return torch.int32, (3, 4) + ((components,) if components != 1 else ()), dict(onehot=levels != 0, levels=levels)
    if kind == 'bits':
        return torch.int32, (3, 4), dict(components=components, onehot=levels != 0, levels=levels)
    return torch.float16, (3, 4, components), dict(onehot=levels != 0, levels=levels)


def test_names_and_kinds_are_the_references():
    assert C.BLOCKS == R.BLOCK_NAMES and C.KINDS == R.KINDS


def test_the_action_descriptor_against_the_reference_table():
    grid = set(REFUSED)
    grid |= set(itertools.product(('f32', 'f64'), (1, 2, 3), (0, 2, 5)))
    grid |= set(itertools.product(('index',), (1, 2), (0, 1, 2, 5, 25, 4096, 4097)))
    grid |= set(itertools.product(('bits',), (0, 1, 3, 8, 16, 17), (0, 2, 3)))
    accepted = refused = 0
    for kind, components, levels in sorted(grid):
        A = R.action_width(kind, components, levels)
        assert C.action_width(kind, components, levels) == A, (kind, components, levels)
        dtype, shape, kw = _inputs(kind, components, levels)
        if A == 0:
            with pytest.raises(ValueError):
                C.descriptor(dtype, shape, **kw)
            refused += 1
        else:
            assert C.descriptor(dtype, shape, **kw) == (kind, components, levels, A), (kind, components, levels)
            accepted += 1
    assert all(R.action_width(*d) == 0 for d in REFUSED) and accepted >= 12 and refused >= len(REFUSED)


def test_the_spellings_a_caller_uses():
    assert C.descriptor(torch.int32, (2, 4), components=8, onehot=True) == ('bits', 8, 2, 16)
    assert C.descriptor(torch.int32, (2, 4), components=8) == ('bits', 8, 0, 8)
    assert C.descriptor(torch.int32, (2, 4), onehot=True, levels=25) == ('index', 1, 25, 25)
    assert C.descriptor(torch.int32, (2, 4)) == ('index', 1, 0, 1)
    assert C.descriptor(torch.float64, (2, 4, 2)) == ('f64', 2, 0, 2)
    for dtype, shape, kw in ((torch.int32, (2, 4), dict(levels=25)), (torch.int32, (2, 4), dict(onehot=True)), (torch.int64, (2, 4), {}),
                             (torch.float32, (2, 4), {}), (torch.float32, (2, 4, 2), dict(components=2)), (torch.int32, (2, 4, 1), dict(components=3)),
                             (torch.float32, (2,), {})):
        with pytest.raises(ValueError):
            C.descriptor(dtype, shape, **kw)


def test_the_width_is_what_the_reference_builds():
    """A of the descriptor == the last axis of central_ref.action_values on encoded actions, for every accepted encoding of the device matrix."""
    rng = np.random.RandomState(2)
    for kind, components, levels in (('f32', 2, 0), ('f64', 2, 0), ('index', 1, 0), ('index', 1, 5), ('index', 1, 25), ('bits', 1, 0), ('bits', 16, 0), ('bits', 3, 2), ('bits', 16, 2)):
        actions = R.encoded_actions(3, 4, kind, components, levels, rng)
        dtype, _, kw = _inputs(kind, components, levels)
        assert torch.as_tensor(actions).dtype == dtype
        got = C.descriptor(dtype, actions.shape, **kw)
        assert got == (kind, components, levels, R.action_values(actions, kind, components, levels, np.float32).shape[-1])


def test_the_column_map_equals_the_references():
    for n, D, S, A, M, joint in LAYOUTS:
        got, want = C.blocks(n, D, S, A, M, joint), R.blocks(n, D, S, A, M, joint)
        assert got == want and list(got[0]) == list(want[0]), (n, D, S, A, M, joint)
    assert C.blocks(3, 7, 2, 2) == R.blocks(3, 7, 2, 2)


def test_the_cyclic_order_is_the_references():
    for n in (1, 2, 3, 8, 16):
        values = np.arange(2 * n, dtype=np.float64).reshape(2, n, 1)
        others = R.others(values)
        assert others.shape == (2, n, n - 1)
        assert np.array_equal(others[0], np.array(C.teammates(n), dtype=np.float64).reshape(n, n - 1))
    assert C.teammates(1) == [[]] and C.teammates(3) == [[1, 2], [2, 0], [0, 1]]
