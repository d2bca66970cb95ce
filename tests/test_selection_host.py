"""Target-selection camera actions (HierarchicalCamera, examples/hrl/wrappers.py of the reference), host side: the fixtures of
tests/golden/make_selection_golden.py are consistent with a NumPy restatement of the wrapper's executor written here -- the same
restatement the GPU tests compare the device executor with --, no recorded camera-frame sits on a branch boundary, the selection
encodings round-trip, and the C ABI carries the new entry points."""
import os
import re

import numpy as np
import pytest

import golden_util as G

FIXTURES = ('selection_4v8-9_multi_s31', 'selection_4v2-9_single_s32', 'selection_2v4-0_multi_s33')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-9


def track_numpy(cam_xy, cam_phi, cam_theta, tgt_xy, selection, view, min_viewing_angle, max_sight_range, rotation_step, zooming_step, area):
    """HierarchicalCamera.executor / .track (wrappers.py:177-220) for the cameras of ONE environment: cam_xy [Nc, 2], cam_phi /
    cam_theta [Nc], tgt_xy [Nt, 2], selection / view [Nc, Nt] bool; `area` = min_viewing_angle * max_sight_range^2, the constant the
    sight range follows from (entities.py:285, 360).  Returns (actions [Nc, 2], margins [Nc]): the smallest relative distance of a
    camera's two branch conditions from equality (inf for a camera without a valid target)."""
    Nc = len(cam_phi)
    actions, margins = np.zeros((Nc, 2)), np.full(Nc, np.inf)
    low = np.asarray([-rotation_step, -zooming_step])
    for c in range(Nc):
        valid = np.flatnonzero(np.logical_and(selection[c], view[c]))
        if len(valid) == 0:
            actions[c] = low
            continue
        center = np.mean([tgt_xy[t] for t in valid], axis=0)
        direction = center - cam_xy[c]
        orientation = np.rad2deg(np.arctan2(direction[-1], direction[0]))
        distance = np.linalg.norm(direction)
        sight_range = np.sqrt(area / cam_theta[c])
        area_product = cam_theta[c] * np.square(sight_range)
        reach = distance * (1.0 + np.sin(np.deg2rad(min_viewing_angle / 2.0)))
        near = np.sqrt(area_product / 180.0) / 2.0
        margins[c] = min(abs(reach - max_sight_range) / max_sight_range, abs(distance - near) / near)
        if reach >= max_sight_range:
            best = min_viewing_angle
        elif distance <= near:
            best = 180.0
        else:
            best = 180.0
            for _ in range(20):
                sr = distance * (1.0 + np.sin(np.deg2rad(min(best / 2.0, 90.0))))
                best = area_product / np.square(sr)
            best = np.clip(best, min_viewing_angle, 180.0)
        delta = (orientation - cam_phi[c] + 180.0) % 360.0 - 180.0
        actions[c] = np.clip([delta, best - cam_theta[c]], low, -low)
    return actions, margins


def metrics_numpy(selection, view):
    """wrappers.py:120-136 for [..., Nc, Nt] bool arrays -> [..., Nc, 4]."""
    selected = selection.sum(axis=-1)
    invalid = np.logical_and(selection, ~view).sum(axis=-1)
    return np.stack([selected, np.logical_and(selection, view).sum(axis=-1), invalid, invalid / np.maximum(1, selected)], axis=-1).astype(np.float64)


def action_mask_numpy(view, multi):
    """wrappers.py:166-175 for [..., Nt] bool -> [..., 2 Nt] / [..., Nt + 1] u8."""
    if multi:
        out = np.repeat(view, 2, axis=-1).astype(np.uint8)
        out[..., ::2] = 1
        return out
    return np.concatenate([view, np.ones(view.shape[:-1] + (1,), dtype=bool)], axis=-1).astype(np.uint8)


def camera_constants(fx):
    return dict(min_viewing_angle=float(fx['camera_min_viewing_angle']), max_sight_range=float(fx['camera_max_sight_range']),
                rotation_step=float(fx['camera_rotation_step']), zooming_step=float(fx['camera_zooming_step']), area=float(fx['camera_area_product']))


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_is_the_numpy_executor_and_no_frame_sits_on_a_branch(name):
    fx = G.load(name + '.npz')
    consts = camera_constants(fx)
    assert consts['area'] == consts['min_viewing_angle'] * consts['max_sight_range'] ** 2
    T = len(fx['step/done'])
    worst, least, tracked = 0.0, np.inf, 0
    for s in range(T):
        cam = fx['step/cam_before'][s]
        # the recorded sight range is the one the executor derives
        assert np.abs(cam[:, 4] - np.sqrt(consts['area'] / cam[:, 3])).max() <= 1e-12 * consts['max_sight_range']
        actions, margins = track_numpy(cam[:, :2], cam[:, 2], cam[:, 3], fx['step/tgt_xy_before'][s], fx['step/selection_bits'][s],
                                       fx['step/view_before'][s], **consts)
        worst = max(worst, np.abs(actions - fx['step/executor_act'][s]).max())
        least = min(least, margins.min())
        tracked += int(np.isfinite(margins).sum())
    assert worst <= 1e-12, worst
    assert least >= MARGIN, least                     # (else: another seed -- the GPU comparison then needs no exclusions)
    assert tracked >= 0.10 * T * int(fx['num_cameras'])
    # what the generator promised: invalid and empty selections in at least 10 % of the camera-frames each
    sel, view = fx['step/selection_bits'], fx['step/view_before']
    assert (~(sel & view).any(axis=-1)).mean() >= 0.10 and (sel & ~view).any(axis=-1).mean() >= 0.10
    # the view a frame acts on is the view the frame before left; metrics and action masks by their definitions
    assert np.array_equal(fx['step/view_before'][1:], fx['step/view_after'][:-1])
    assert np.array_equal(fx['step/view_before'][0], fx['reset/camera_target_view_mask'])
    assert np.array_equal(fx['step/metrics'], metrics_numpy(sel, fx['step/view_after']))
    multi = bool(fx['multi_selection'])
    last = np.cumsum(fx['skip/frames']) - 1
    assert np.array_equal(fx['skip/action_mask'], action_mask_numpy(fx['step/view_after'][last], multi))
    assert np.array_equal(fx['reset/action_mask'], action_mask_numpy(fx['reset/camera_target_view_mask'], multi))
    # the wrapper's fragment: rewards summed, metrics averaged over the frames that ran
    K = int(fx['frame_skip'])
    for ls, n in enumerate(fx['skip/frames']):
        frames = np.flatnonzero(fx['step/learner_step'] == ls)
        assert len(frames) == n and (n == K or fx['step/done'][frames[-1]])
        if K > 1:
            np.testing.assert_allclose(fx['skip/reward_cam'][ls], fx['step/shaped_reward_cam'][frames].sum(axis=0), rtol=0, atol=1e-12)
            np.testing.assert_allclose(fx['skip/info_metrics'][ls], fx['step/metrics'][frames].mean(axis=0), rtol=0, atol=1e-12)
    if name == 'selection_2v4-0_multi_s33':            # the episode ends INSIDE a fragment
        assert fx['step/done'][-1] and 0 < fx['skip/frames'][-1] < K


def test_selection_encodings():
    """mate_amd.engine.encode_selection / decode_selection on the CPU: a multi-selection packs to bit t for target t and comes back;
    a single selection's index decodes to the wrapper's index2onehot row (wrappers.py:64), row Nt all zero; packed words and
    indices pass through; shapes and dtypes are refused, values are not."""
    import torch
    from mate_amd.engine import decode_selection, encode_selection
    N, Nc, Nt = 5, 4, 8
    rng = np.random.RandomState(0)
    bits = rng.random_sample((N, Nc, Nt)) < 0.5
    words = encode_selection(torch.from_numpy(bits.astype(np.int64)), True, N, Nc, Nt)
    assert words.dtype == torch.int32 and words.shape == (N, Nc)
    assert np.array_equal(words.numpy(), (bits.astype(np.int64) << np.arange(Nt)).sum(axis=-1))
    assert np.array_equal(decode_selection(words, True, Nt).numpy(), bits)
    assert torch.equal(encode_selection(words, True, N, Nc, Nt), words)              # (packed words as they are)
    assert np.array_equal(decode_selection(words | (1 << 20), True, Nt).numpy(), bits)      # (bits beyond Nt are ignored)
    full = encode_selection(torch.ones((1, 1, 16), dtype=torch.uint8), True, 1, 1, 16)
    assert int(full) == 0xffff and decode_selection(full, True, 16).all()
    onehot = np.eye(Nt + 1, Nt, dtype=bool)          # index2onehot
    index = np.concatenate([np.arange(Nt + 1), rng.randint(0, Nt + 1, size=N * Nc - Nt - 1)]).reshape(N, Nc)
    single = encode_selection(torch.from_numpy(index), False, N, Nc, Nt)
    assert single.dtype == torch.int32 and np.array_equal(single.numpy(), index)
    decoded = decode_selection(single, False, Nt).numpy()
    assert np.array_equal(decoded, onehot[index])
    assert not decoded.reshape(-1, Nt)[Nt].any()      # (index Nt: nothing selected)
    assert not decode_selection(torch.tensor([-1, Nt + 3]), False, Nt).any()
    for bad in (torch.zeros((N, Nc), dtype=torch.float32), torch.zeros((N, Nc + 1), dtype=torch.int32), torch.zeros((N, Nc, Nt + 1), dtype=torch.int64)):
        with pytest.raises(AssertionError):
            encode_selection(bad, True, N, Nc, Nt)
    with pytest.raises(AssertionError):
        encode_selection(torch.zeros((N, Nc, Nt), dtype=torch.int64), False, N, Nc, Nt)
    # the restatements the GPU tests compare with, on the decoded bits
    view = rng.random_sample((N, Nc, Nt)) < 0.5
    m = metrics_numpy(decode_selection(words, True, Nt).numpy(), view)
    assert np.array_equal(m[..., 0], m[..., 1] + m[..., 2]) and (m[..., 3] <= 1).all()
    assert action_mask_numpy(view, True).shape == (N, Nc, 2 * Nt) and action_mask_numpy(view, False)[..., -1].all()


def test_c_abi_declares_and_exports_the_selection_entry_points():
    from mate_amd import _native
    with open(os.path.join(ROOT, 'include', 'mate_engine.h')) as fh:
        declared = set(re.findall(r'\b(mate_engine_[a-z_]+)\s*\(', fh.read()))
    for name in ('mate_engine_enable_selection', 'mate_engine_disable_selection', 'mate_engine_step_selected', 'mate_engine_selection_actions'):
        assert name in declared and name in _native.EXPORTED_SYMBOLS, name
