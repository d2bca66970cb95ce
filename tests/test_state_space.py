"""Host side of the global state rows: the state-space bounds, the affine table of the fused normalisation against the reference's
own normalize_observation (tests/golden/state_norm.npz), and the C ABI's new symbols.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import golden_util as G

NORM = G.load('state_norm.npz')
TRACES = [str(n) for n in NORM['traces']]


@pytest.mark.parametrize('name', TRACES)
def test_state_space_and_affine_table_against_the_reference(name):
    from mate_amd import constants as C
    from mate_amd.spaces import rescale_affine
    fx = G.load(name + '.npz')
    nums = (int(fx['num_cameras']), int(fx['num_targets']), int(fx['num_obstacles']))
    space = C.state_space_of(*nums)
    assert space.shape == (13 + 9 * nums[0] + 14 * nums[1] + 3 * nums[2] + 2 * nums[1] + 16,)
    assert np.array_equal(space.low, NORM[name + '/low']) and np.array_equal(space.high, NORM[name + '/high'])
    # no element unbounded below, none degenerate; the freight / bounty / cargo tail is bounded below only
    tail = 2 * nums[1] + 16
    assert np.all(np.isfinite(space.low)) and np.all(space.high > space.low)
    assert np.all(space.low[-tail:] == 0.0) and np.all(np.isinf(space.high[-tail:]))
    scale, bias = rescale_affine(space)
    both = np.isfinite(space.high)
    assert np.array_equal(scale[~both], np.ones(int((~both).sum()))) and np.array_equal(bias[~both], -space.low[~both])
    steps = NORM[name + '/step']
    raw = np.concatenate([fx['reset/state'][None], fx['step/state'][:len(steps)]]).astype(np.float64)
    ref = np.concatenate([NORM[name + '/reset'][None], steps])
    assert np.all(np.isfinite(ref))
    err = np.abs(scale * raw + bias - ref)
    assert err.max() <= 1e-12, (name, err.max())
    # the normalised box, as RLlibMultiAgentCentralizedTraining derives it: the map applied to the bounds
    norm_space = C.normalized_state_space_of(*nums)
    assert np.array_equal(norm_space.low[both], -np.ones(int(both.sum()))) and np.array_equal(norm_space.high[both], np.ones(int(both.sum())))
    assert np.array_equal(norm_space.low[~both], np.zeros(int((~both).sum()))) and np.all(np.isinf(norm_space.high[~both]))


def test_environment_state_space_is_the_shared_one():
    """_ScenarioMixin._setup_spaces takes its box from constants.state_space_of."""
    from mate_amd import constants as C
    from mate_amd.environment import _ScenarioMixin

    class Probe(_ScenarioMixin):
        def __init__(self):
            self._setup_scenario('MATE-4v8-9.yaml', {})
            self.num_cameras, self.num_targets, self.num_obstacles = 4, 8, 9
            self._setup_spaces()

    probe = Probe()
    ref = C.state_space_of(4, 8, 9)
    assert probe.state_space.shape == (220,)
    assert np.array_equal(probe.state_space.low, ref.low) and np.array_equal(probe.state_space.high, ref.high)


def test_observation_rescale_uses_the_same_affine_rule():
    """The helper factored out of Engine.set_obs_transform: [-1, 1] where bounded on both sides, shifted where bounded below only."""
    from mate_amd import constants as C
    from mate_amd.spaces import rescale_affine
    space = C.camera_observation_space_of(4, 8, 9)
    scale, bias = rescale_affine(space)
    both = np.isfinite(space.low) & np.isfinite(space.high) & (space.high > space.low)
    assert np.allclose(scale[both] * space.low[both] + bias[both], -1.0, atol=1e-15)
    assert np.allclose(scale[both] * space.high[both] + bias[both], 1.0, atol=1e-15)
    below_only = np.isfinite(space.low) & ~np.isfinite(space.high)
    assert np.array_equal(scale[below_only], np.ones(int(below_only.sum()))) and np.array_equal(bias[below_only], -space.low[below_only])


def test_library_exports_the_state_row_entry_points():
    from mate_amd import _native
    assert os.path.exists(_native.LIB_PATH), 'run __graft_entry__.build() first'
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ('mate_engine_enable_state_rows', 'mate_engine_state_rows'):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name
    with open(os.path.join(os.path.dirname(_native.LIB_PATH), 'kernel_resources.json')) as fh:
        import json
        kernels = {k: v for k, v in json.load(fh).items() if 'state_rows_kernel' in k}
    assert len(kernels) == 2 and all(v['ScratchSize'] == 0 for v in kernels.values()), kernels
