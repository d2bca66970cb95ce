"""The host-side tables of the centralised-training rows: the row the reference's RLlibMultiAgentCentralizedTraining hands
each agent of one team is `obs | state | the teammates' previous actions in cyclic order | [action_mask] | [the teammates' observations]`.

Pure Python, no engine and no device: the action descriptor a learner's action tensor stands for, the width of one teammate's entry, and the column
map (the models' `flat_obs_slices`).  There is NO device launch for the rows (DESIGN.md 3.18 says why); a learner that assembles them itself, and
whoever writes the launch, take the layout from here.  Held to tests/central_ref.py, which is pinned to the reference's own recordings."""
import torch

BLOCKS = ('obs', 'state', 'prev_others_joint_action', 'action_mask', 'others_joint_observation')
KINDS = {'f32': 0, 'f64': 1, 'index': 2, 'bits': 3}      # the source kinds of the action descriptor (kind, components, levels)
MAX_LEVELS, MAX_COMPONENTS = 4096, 16


def action_width(kind, components, levels):
    """A of one teammate's entry in the action block, or 0 for a descriptor that has no encoding:
    'f32' / 'f64'  a continuous pair (components 2, levels 0): 2;
    'index'        an int32 index (components 1) as a number (levels 0): 1, or one-hot over `levels` in 2..4096: levels;
    'bits'         the low `components` (1..16) bits of an int32 word, each as 0 / 1 (levels 0): components, or as [1 - b, b] pairs (levels 2): 2 components."""
    if kind in ('f32', 'f64'):
        return 2 if components == 2 and levels == 0 else 0
    if kind == 'index':
        return 0 if components != 1 else 1 if levels == 0 else levels if 2 <= levels <= MAX_LEVELS else 0
    if kind == 'bits':
        return 0 if not 1 <= components <= MAX_COMPONENTS else components if levels == 0 else 2 * components if levels == 2 else 0
    return 0


def descriptor(dtype, shape, onehot=False, levels=0, components=None):
    """(kind, components, levels, A) of an action tensor, from its dtype and its [N, n, ...] shape: float32 / float64 [N, n, 2] is a continuous pair;
    int32 [N, n] is an index -- as a number, or `onehot` over `levels` -- or, with `components` = c, the low c bits of a selection word, each as 0 / 1
    or, `onehot`, as a [1 - b, b] pair.  `levels` belongs to `onehot`.  ValueError for what has no encoding."""
    shape = tuple(int(v) for v in shape)
    trailing = shape[2:]
    levels = int(levels)
    if not onehot and levels != 0:
        raise ValueError(f'levels = {levels} belongs to onehot=True')
    if dtype in (torch.float32, torch.float64):
        kind = 'f32' if dtype == torch.float32 else 'f64'
        comps = trailing[0] if len(trailing) == 1 and components is None else 0
        levels = (levels or 2) if onehot else 0
    elif dtype == torch.int32 and components is not None:
        kind, comps = 'bits', int(components) if not trailing else 0
        levels = (levels or 2) if onehot else 0
    elif dtype == torch.int32:
        kind, comps = 'index', 1 + len(trailing)
        levels = (levels or 1) if onehot else 0
    else:
        raise ValueError(f'actions of {dtype}: float32 / float64 [N, n, 2] or int32 [N, n]')
    A = action_width(kind, comps, levels) if len(shape) >= 2 else 0
    if A == 0:
        raise ValueError(f'no action block for {dtype} actions of shape {shape} with onehot = {bool(onehot)}, levels = {levels}, components = {components}: '
                         f'float32 / float64 [N, n, 2]; int32 [N, n] as a number or one-hot over 2..{MAX_LEVELS} levels; int32 [N, n] with components in '
                         f'1..{MAX_COMPONENTS} (one-hot: [1 - b, b] pairs)')
    return kind, comps, levels, A


def blocks(n, D, S, A, M=0, joint=False):
    """({block name: column slice}, W) of the rows of a team of n agents in the wrapper's OrderedDict order: obs (D) | state (S) |
    prev_others_joint_action ((n - 1) A) | [action_mask (M)] | [others_joint_observation ((n - 1) D)], the two optional blocks only where they exist."""
    widths = (D, S, (n - 1) * A, M, (n - 1) * D if joint else 0)
    out, at = {}, 0
    for name, w in zip(BLOCKS, widths):
        if w or name in BLOCKS[:3]:
            out[name] = slice(at, at + w)
        at += w
    return out, at


def teammates(n):
    """[n][n - 1]: agent a's k-th teammate in both "others" blocks is (a + 1 + k) % n (the wrapper's cycled[i + 1 : i + n])."""
    return [[(a + 1 + k) % n for k in range(n - 1)] for a in range(n)]
