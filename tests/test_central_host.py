"""Host-side tests of the centralised-training rows, no GPU: the NumPy builder of tests/central_ref.py against what the
reference's environment under the trainers' chain and the wrapper's stand-in recorded (tests/golden/central_*.npz, tests/golden/make_central_golden.py),
exactly, and the column map.  There is no device launch yet (DESIGN.md section 3.18 says why): these pin what one has to write."""
import os

import numpy as np
import pytest

import central_ref as R
import golden_util as G

FIXTURES = {      # name -> (learner, action kind, joint observation, action mask)
    'central_4v8-9_camera_joint': ('camera', 'f64', True, False),
    'central_2v4-0_target_discrete': ('target', 'index', False, False),
    'central_4v8-9_hierarchical': ('camera', 'bits', False, True),
}
LARGEST_OTHER_FIXTURE = max(os.path.getsize(os.path.join(G.GOLDEN_DIR, f)) for f in os.listdir(G.GOLDEN_DIR) if f.endswith('.npz') and not f.startswith('central_'))


def fixture_actions(fx, t, kind):
    """The persistent action tensor [1, n, ...] as it stands when row t is built: the joint action of the last step that ran (a reset row keeps it)."""
    while t > 0 and fx['step/reset'][t]:
        t -= 1
    action = fx['step/action'][t]
    if kind == 'bits':
        action = (action.astype(np.int64) << np.arange(action.shape[-1])).sum(axis=-1)
    return action[None].astype(np.float64 if kind == 'f64' else np.int32)


@pytest.mark.parametrize('name', sorted(FIXTURES))
def test_central_ref_reproduces_the_recorded_reference(name):
    """Every recorded row, the reset() rows included: the concatenation of the wrapper's blocks in its OrderedDict order, exactly.  The action tensor
    holds the last step's joint action at a reset row, as a persistent tensor does: the zeros come from the episode-step rule."""
    learner, kind, joint, masked = FIXTURES[name]
    fx = G.load(name + '.npz')
    assert str(fx['learner_team']) == learner and bool(fx['joint_observation']) == joint and bool(fx['hierarchical']) == masked
    n = int(fx['num_cameras'] if learner == 'camera' else fx['num_targets'])
    Nt = int(fx['num_targets'])
    T, D, S = len(fx['step/done']), fx['step/obs'].shape[-1], fx['step/state'].shape[-1]
    components = {'f64': 2, 'index': 1, 'bits': Nt}[kind]
    A = R.action_width(kind, components, 0)
    M = fx['row/action_mask'].shape[-1] if masked else 0
    names = [str(b) for b in fx['block_names']]
    layout, W = R.blocks(n, D, S, A, M, joint)
    assert names == list(layout) == [b for b in R.BLOCK_NAMES if 'row/' + b in fx]
    assert int(fx['step/done'].sum()) == 1 and int(fx['step/reset'].sum()) == 2 and fx['step/reset'][0] and not fx['step/reset'][-1]
    done_at = int(np.flatnonzero(fx['step/done'])[0])
    assert fx['step/reset'][done_at + 1] and done_at + 2 < T          # through the episode end and the reset() behind it
    for t in range(T):
        expected = np.concatenate([fx['row/' + b][t].astype(np.float64) for b in names], axis=-1)
        assert expected.shape == (n, W)
        epstep = 0 if fx['step/reset'][t] else 1
        rows = R.build(fx['step/obs'][t][None], fx['step/state'][t][None], fixture_actions(fx, t, kind), [epstep], kind, components, 0,
                       mask=fx['row/action_mask'][t][None] if masked else None, joint=joint, dtype=np.float64)
        assert np.array_equal(rows[0], expected), (name, t)
        if fx['step/reset'][t]:
            assert not rows[0][:, layout['prev_others_joint_action']].any()
            if t:                                                        # ... and `shift` brings the tensor's content back without the rule
                shifted = R.shift(rows, fixture_actions(fx, t, kind), kind, components, 0, D, S)
                assert np.array_equal(shifted[0], np.concatenate([fx['row/' + b][t - 1].astype(np.float64) if b == 'prev_others_joint_action' else
                                                                  fx['row/' + b][t].astype(np.float64) for b in names], axis=-1))
        else:
            assert rows[0][:, layout['prev_others_joint_action']].any() or kind != 'f64'
    # the cyclic order, said once more without the builder: agent a's k-th teammate is (a + 1 + k) % n
    t = done_at
    block = fx['row/prev_others_joint_action'][t].reshape(n, n - 1, A)
    action = R.action_values(fixture_actions(fx, t, kind), kind, components, 0, np.float64)[0]
    for a in range(n):
        for k in range(n - 1):
            assert np.array_equal(block[a, k], action[(a + 1 + k) % n])
    for key in fx:
        assert fx[key].dtype.kind in 'fiubU', key                      # arrays and names only
    assert os.path.getsize(os.path.join(G.GOLDEN_DIR, name + '.npz')) <= LARGEST_OTHER_FIXTURE


def test_onehot_forms_and_the_column_map():
    """One-hot encodings from the raw ones; the column map against the block widths; encoded inputs tell every source element apart."""
    rng = np.random.RandomState(5)
    index = R.encoded_actions(3, 4, 'index', 1, 25, rng)
    hot = R.action_values(index, 'index', 1, 25, np.float32)
    assert hot.shape == (3, 4, 25) and (hot.sum(-1) == 1).all() and np.array_equal(hot.argmax(-1), index)
    bits = R.encoded_actions(3, 4, 'bits', 8, 2, rng)
    raw, pairs = R.action_values(bits, 'bits', 8, 0, np.float64), R.action_values(bits, 'bits', 8, 2, np.float64)
    assert raw.shape == (3, 4, 8) and pairs.shape == (3, 4, 16)
    assert np.array_equal(pairs[..., 1::2], raw) and np.array_equal(pairs[..., 0::2], 1 - raw)
    assert np.array_equal((raw.astype(np.int64) << np.arange(8)).sum(-1), bits)
    for n, D, S, A, M, joint in ((4, 145, 153, 2, 0, True), (8, 113, 153, 25, 0, False), (4, 145, 153, 16, 16, True), (1, 20, 43, 2, 0, True), (7, 33, 151, 1, 6, False)):
        layout, W = R.blocks(n, D, S, A, M, joint)
        widths = {'obs': D, 'state': S, 'prev_others_joint_action': (n - 1) * A, 'action_mask': M, 'others_joint_observation': (n - 1) * D if joint else 0}
        assert W == sum(widths.values()) and list(layout) == [b for b in R.BLOCK_NAMES if widths[b] or b in R.BLOCK_NAMES[:3]]
        at = 0
        for b in layout:
            assert layout[b] == slice(at, at + widths[b])
            at += widths[b]
        assert at == W
    obs = R.encoded_obs(5, 3, 7, np.float32, first_env=2)
    assert len(np.unique(obs)) == obs.size
    rows = R.build(obs, np.zeros((5, 2), np.float64), R.encoded_actions(5, 3, 'f32', 2, 0, rng), np.ones(5), 'f32', 2, 0, joint=True)
    assert rows.dtype == np.float32 and rows.shape == (5, 3, 7 + 2 + 4 + 14)
    assert np.array_equal(rows[4, 2, -14:-7], obs[4, 0]) and np.array_equal(rows[4, 2, -7:], obs[4, 1]) and np.array_equal(rows[1, 0, 9:11], [(16 + 1) * 2 + 0.5, (16 + 1) * 2 + 1.5])
    one = R.build(obs[:, :1], np.zeros((5, 2)), np.zeros((5, 1, 2)), np.ones(5), 'f64', 2, 0, joint=True)
    assert one.shape == (5, 1, 9)                                      # n = 1: both "others" blocks are empty
    for kind, components, levels in (('f32', 2, 2), ('f64', 3, 0), ('index', 2, 0), ('index', 1, 1), ('bits', 0, 0), ('bits', 17, 0), ('bits', 4, 3), ('pair', 2, 0)):
        assert R.action_width(kind, components, levels) == 0
