"""Observation/action space descriptors.  Uses `gym.spaces` when gym is installed (so reference
wrappers see real gym spaces) and an attribute-compatible minimal stand-in otherwise."""
import numpy as np

try:  # pragma: no cover - depends on the user's environment
    from gym import spaces as _gym_spaces
    Box, Tuple, Discrete = _gym_spaces.Box, _gym_spaces.Tuple, _gym_spaces.Discrete
    HAVE_GYM = True
except Exception:  # gym missing (as in the build image)
    HAVE_GYM = False

    class _Space:
        def __init__(self):
            self._rng = np.random.RandomState()

        def seed(self, seed=None):
            self._rng = np.random.RandomState(seed)
            return [seed]

        @property
        def np_random(self):
            return self._rng

        def __contains__(self, x):
            return self.contains(x)

    class Box(_Space):
        def __init__(self, low, high, shape=None, dtype=np.float64):
            super().__init__()
            self.dtype = np.dtype(dtype)
            if shape is None:
                shape = np.broadcast(np.asarray(low), np.asarray(high)).shape
            self.low = np.broadcast_to(np.asarray(low, dtype=self.dtype), shape).copy()
            self.high = np.broadcast_to(np.asarray(high, dtype=self.dtype), shape).copy()
            self.shape = tuple(shape)

        def sample(self):
            lo = np.where(np.isfinite(self.low), self.low, -1e6)
            hi = np.where(np.isfinite(self.high), self.high, 1e6)
            return self._rng.uniform(lo, hi).astype(self.dtype)

        def contains(self, x):
            x = np.asarray(x)
            return x.shape == self.shape and bool(np.all(x >= self.low) and np.all(x <= self.high))

        def __repr__(self):
            return f'Box({self.low.min()}, {self.high.max()}, {self.shape}, {self.dtype})'

    class Discrete(_Space):
        def __init__(self, n):
            super().__init__()
            self.n = int(n)
            self.shape = ()
            self.dtype = np.dtype(np.int64)

        def sample(self):
            return int(self._rng.randint(self.n))

        def contains(self, x):
            return 0 <= int(x) < self.n

    class Tuple(_Space):
        def __init__(self, spaces):
            super().__init__()
            self.spaces = tuple(spaces)

        def seed(self, seed=None):
            out = super().seed(seed)
            for i, space in enumerate(self.spaces):
                space.seed(None if seed is None else seed + i + 1)
            return out

        def sample(self):
            return tuple(space.sample() for space in self.spaces)

        def contains(self, x):
            return len(x) == len(self.spaces) and all(s.contains(v) for s, v in zip(self.spaces, x))

        def __getitem__(self, i):
            return self.spaces[i]

        def __len__(self):
            return len(self.spaces)

        def __iter__(self):
            return iter(self.spaces)


def rescale_affine(space):
    """(scale, bias) with `scale * x + bias` == mate.normalize_observation(x, space) (mate/agents/utils.py:97-127 of the reference):
    subtract `low` where the box is bounded below, then `2 x / (high - low) - 1` where it is bounded on both sides and `high > low`."""
    low, high = np.asarray(space.low, dtype=np.float64), np.asarray(space.high, dtype=np.float64)
    scale, bias = np.ones_like(low), np.zeros_like(low)
    below = np.isfinite(low)
    both = below & np.isfinite(high) & (high > low)
    bias[below] = -low[below]                      # rescaled[bounded_below] -= low
    span = np.where(both, high - low, 1.0)
    scale[both] = 2.0 / span[both]                 # rescaled[mask] = 2 * rescaled / (high - low) - 1
    bias[both] = -2.0 * low[both] / span[both] - 1.0
    return np.ascontiguousarray(scale), np.ascontiguousarray(bias)


def fragment_column_table(team, num_cameras, num_targets, num_obstacles, relative_coordinates=False, rescaled_observation=False):
    """The per-column table of the fragment launch (mate_engine_enable_fragment_rows) for one team's observation row [D]:
    `(sub, flag, scale, bias)` with out = ((v - own x) where sub = 1, (v - own y) where 2, v where 0; +0 where flag >= 0 and that
    column of the row reads 0) * scale + bias -- RelativeCoordinates then RescaledObservation (mate/agents/utils.py:40-137 of the
    reference) on a PLAIN row, with the packer's visible / invisible rule: the entries of an entity the agent does not see stay 0
    through the subtraction.  The row owner's (x, y) are columns 13 and 14 (the head of its own state, behind the 13 preserved
    entries).  Coordinates: the four warehouse centres of the preserved block (columns 4 .. 11, never gated) and x, y at the head
    of every opponent / obstacle / teammate entry, gated by that entry's flag (its last column).  None when neither wrapper is asked for."""
    from mate_amd import constants as consts
    assert team in ('camera', 'target')
    if not relative_coordinates and not rescaled_observation:
        return None
    nums = (num_cameras, num_targets, num_obstacles)
    camera = team == 'camera'
    space = consts.camera_observation_space_of(*nums) if camera else consts.target_observation_space_of(*nums)
    D = int(np.prod(space.shape))
    self_dim = 9 if camera else 14
    blocks = ((num_targets, 5), (num_obstacles, 4), (num_cameras, 7)) if camera else ((num_cameras, 7), (num_obstacles, 4), (num_targets, 5))
    assert D == 13 + self_dim + sum(count * width for count, width in blocks), (D, team, nums)
    sub, flag = np.zeros(D, dtype=np.int32), np.full(D, -1, dtype=np.int32)
    if relative_coordinates:
        sub[4:12:2], sub[5:12:2] = 1, 2
    start = 13 + self_dim
    for count, width in blocks:
        for entry in range(count):
            flag[start:start + width] = start + width - 1
            if relative_coordinates:
                sub[start], sub[start + 1] = 1, 2
            start += width
    scale, bias = rescale_affine(space) if rescaled_observation else (np.ones(D), np.zeros(D))
    return sub, flag, np.ascontiguousarray(scale, dtype=np.float64), np.ascontiguousarray(bias, dtype=np.float64)


def apply_fragment_column_table(rows, table):
    """`fragment_column_table` applied to plain rows [..., D] in NumPy, in the launch's order of operations (the tests' restatement)."""
    rows = np.asarray(rows)
    if table is None:
        return rows.copy()
    sub, flag, scale, bias = table
    own = np.stack([np.zeros_like(rows[..., 0]), rows[..., 13], rows[..., 14]], axis=-1)[..., sub]
    visible = np.where(flag >= 0, rows[..., np.maximum(flag, 0)] != 0, True)
    gated = np.where(visible, rows - own, np.zeros_like(rows))
    return gated * scale.astype(rows.dtype) + bias.astype(rows.dtype)


def _square_grid(levels):
    """`levels` x `levels` grid on [-1, 1]^2, x fastest (np.meshgrid of two linspaces, discrete_action_spaces.py:107-113)."""
    if not (isinstance(levels, (int, np.integer)) and levels >= 3 and levels % 2 == 1):
        raise AssertionError(f'The discrete level must be an odd number that not less than 3. Got levels = {levels}.')
    axis = np.linspace(start=-1.0, stop=+1.0, num=levels, endpoint=True)
    return np.stack(np.meshgrid(axis, axis), axis=-1).reshape(-1, 2)


def camera_action_grid(levels):
    """Normalised action grid of the reference's DiscreteCamera wrapper (discrete_action_spaces.py:98-117):
    action = action_space.high * grid[index]."""
    return _square_grid(levels)


def target_action_grid(levels):
    """Normalised action grid of DiscreteTarget (discrete_action_spaces.py:204-228): the square grid pulled
    onto the unit disc along each ray, so that every direction has the same maximum step."""
    grid = _square_grid(levels)
    angle = np.arctan2(grid[..., -1], grid[..., 0])
    bound = 1.0 / np.cos(np.pi * ((angle / np.pi + 0.25) % 0.5 - 0.25))
    return grid / bound[..., np.newaxis]
