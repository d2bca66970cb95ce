"""NumPy reference of the centralised-training rows: the rows of one team from (obs, state, actions, mask, epstep) for every
action encoding, the `shift` form, the column map, and encoded inputs that tell environment, agent and column apart.  Pinned to the reference's own wrapper
by tests/test_central_host.py (tests/golden/central_*.npz); what a device launch will be held to, bit for bit."""
import numpy as np

BLOCK_NAMES = ('obs', 'state', 'prev_others_joint_action', 'action_mask', 'others_joint_observation')
KINDS = {'f32': 0, 'f64': 1, 'index': 2, 'bits': 3}      # the source kinds of the action descriptor (kind, components, levels)


def action_width(kind, components, levels):
    """A of one teammate's action block, or 0 for a combination the engine refuses."""
    if kind in ('f32', 'f64'):
        return 2 if components == 2 and levels == 0 else 0
    if kind == 'index':
        return 0 if components != 1 else 1 if levels == 0 else levels if 2 <= levels <= 4096 else 0
    if kind == 'bits':
        return 0 if not 1 <= components <= 16 else components if levels == 0 else 2 * components if levels == 2 else 0
    return 0


def blocks(n, D, S, A, M=0, joint=False):
    """{name: column slice} of the layout, in the wrapper's OrderedDict order (the two optional blocks only where they exist), and W."""
    widths = (D, S, (n - 1) * A, M, (n - 1) * D if joint else 0)
    out, at = {}, 0
    for name, w in zip(BLOCK_NAMES, widths):
        if w or name in BLOCK_NAMES[:3]:
            out[name] = slice(at, at + w)
        at += w
    return out, at


def action_values(actions, kind, components, levels, dtype):
    """[N, n, A] numbers of `dtype`: what one agent's action contributes to its teammates' rows."""
    actions = np.asarray(actions)
    if kind in ('f32', 'f64'):
        return actions.astype(dtype)
    word = actions.astype(np.int64)
    if kind == 'index':
        return word[..., None].astype(dtype) if levels == 0 else (word[..., None] == np.arange(levels)).astype(dtype)
    bits = (word[..., None] >> np.arange(components)) & 1
    if levels == 0:
        return bits.astype(dtype)
    return np.stack([1 - bits, bits], axis=-1).reshape(bits.shape[:-1] + (2 * components,)).astype(dtype)


def others(values):
    """[N, n, X] -> [N, n, (n - 1) X]: for agent a the entries of its teammates (a + 1 + k) % n, k = 0 .. n - 2."""
    N, n = values.shape[:2]
    if n == 1:
        return np.zeros((N, 1, 0), dtype=values.dtype)
    order = (np.arange(n)[:, None] + 1 + np.arange(n - 1)[None, :]) % n
    return values[:, order].reshape(N, n, -1)


def build(obs, state, actions, epstep, kind, components, levels, mask=None, joint=False, dtype=None):
    """The rows [N, n, W]: obs | state | the teammates' actions (zeros where epstep == 0) | [mask as 0 / 1] | [the teammates' observations]."""
    obs = np.asarray(obs)
    dtype = dtype or obs.dtype
    N, n, _ = obs.shape
    act = action_values(actions, kind, components, levels, dtype)
    act = np.where((np.asarray(epstep).reshape(N) == 0)[:, None, None], np.zeros((), dtype=dtype), act)
    parts = [obs.astype(dtype), np.broadcast_to(np.asarray(state).astype(dtype)[:, None, :], (N, n, np.asarray(state).shape[-1])), others(act)]
    if mask is not None:
        parts.append((np.asarray(mask) != 0).astype(dtype))
    if joint:
        parts.append(others(obs.astype(dtype)))
    return np.ascontiguousarray(np.concatenate(parts, axis=-1))


def shift(rows, actions, kind, components, levels, D, S):
    """`rows` with the prev_others_joint_action block alone rewritten from `actions`, no zeros for a fresh episode (ShiftAgentActionTimestep)."""
    out = np.array(rows, copy=True)
    block = others(action_values(actions, kind, components, levels, rows.dtype))
    out[:, :, D + S:D + S + block.shape[-1]] = block
    return out


def encoded_obs(N, n, D, dtype, first_env=0):
    """Observation rows whose every element names (environment, agent, column): exact in f32 up to 2^24."""
    e, a, c = np.meshgrid(np.arange(N) + first_env, np.arange(n), np.arange(D), indexing='ij')
    return ((e * 16 + a) * 1024 + c + 1).astype(dtype)


def encoded_actions(N, n, kind, components, levels, rng):
    """Actions that differ between every two agents of an environment where the encoding allows it, and between environments."""
    if kind in ('f32', 'f64'):
        e, a, c = np.meshgrid(np.arange(N), np.arange(n), np.arange(2), indexing='ij')
        return ((e * 16 + a) * 2 + c + 0.5).astype(np.float32 if kind == 'f32' else np.float64)
    if kind == 'index':
        top = levels if levels else 25
        return ((np.arange(N)[:, None] * 7 + np.arange(n)[None, :] * 3 + 1) % top).astype(np.int32)
    return rng.randint(0, 1 << components, size=(N, n)).astype(np.int32)
