"""Host side of the per-frame FrameSkip fragments (csrc/frame_rows.hpp): the NumPy restatement of the per-frame
rule (tests/frame_fragment_ref.py) fed, frame by frame, the recorded frames of tests/golden/fragment_*.npz against the recorded FrameSkip
outputs -- within the bars tests/test_gpu_fragment.py derives for fixtures --, the first-rows form, the header, the ABI version, the
argument rules of fragment_arguments(per_frame=True), and the unchanged refusals without it.  No GPU."""
import os
import re

import numpy as np
import pytest

import frame_fragment_ref as R
import golden_util as G
from test_fragment_host import FIXTURES, REFUSED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 37


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_frame_by_frame(name):
    fx = G.load(name + '.npz')
    K = int(fx['frame_skip'])
    rows, scalars, which = R.fixture_frames(fx, N)
    A, D = rows.shape[2:]
    st = R.new_state(N, A, D, sentinel=777.0)
    st['rewards'][...] = 5.0                               # phase 0 overwrites: whatever the tensors held
    st['frames'][...] = 9
    for f in range(K):
        R.fold_frame(st, scalars[f], rows[f], f, K)
    counts = fx['skip/frames'][which]
    assert (counts < K).any() and (counts == K).any()      # both kinds of fragment in every fixture
    R.check_fixture(name, st, fx, which)


def test_an_idle_fragment_and_the_first_rows_form():
    K, A, D = 3, 2, 5
    rng = np.random.default_rng(3)
    scalars = rng.random((K, 4, 8)).astype(np.float32)
    scalars[:, :, 2] = [[0, 0, 2, 0], [0, 1, 2, 0], [0, 2, 2, 1]]      # env 0 runs through, 1 ends on frame 1, 2 idles, 3 ends on the last
    rows = rng.random((K, 4, A, D))
    st = R.new_state(4, A, D, sentinel=-1.0)
    for f in range(K):
        R.fold_frame(st, scalars[f], rows[f], f, K, reward_rows=rows[f][:, :, 0])
    assert st['frames'].tolist() == [3, 2, 0, 3] and st['done'].tolist() == [0, 1, 0, 1]
    assert (st['obs'][2] == -1.0).all() and (st['rewards'][2] == 0).all() and (st['info'][2] == 0).all() and (st['shaped'][2] == 0).all()
    assert np.array_equal(st['obs'][1], rows[1, 1]) and np.array_equal(st['obs'][0], rows[2, 0])
    assert st['info'][1, 0] == (np.float64(scalars[0, 1, 3]) + np.float64(scalars[1, 1, 3])) / 2
    assert st['shaped'][1, 0] == rows[0, 1, 0, 0] + rows[1, 1, 0, 0]
    first = rng.random((4, A, D))
    kept = st['obs'].copy()
    R.first_rows(st, scalars[K - 1], first)
    assert st['restarted'].tolist() == [0, 1, 1, 1]
    assert np.array_equal(st['obs'][1:], first[1:]) and np.array_equal(st['final_obs'][1:], kept[1:]) and np.array_equal(st['obs'][0], kept[0])


def test_header_abi_and_bindings():
    from mate_amd import _native
    with open(os.path.join(ROOT, 'include', 'mate_engine.h')) as fh:
        header = fh.read()
    assert re.search(r'#define\s+MATE_ABI_VERSION\s+1\b', header)
    body = re.search(r'typedef\s+struct\s*\{([^{}]*)\}\s*mate_frame_fragments\s*;', header).group(1)
    members = re.findall(r'(\w+)\s*(?:;|,)', re.sub(r'/\*.*?\*/', '', body, flags=re.S))
    assert members == [name for name, _ in _native.MateFrameFragments._fields_]
    assert set(members) >= {'team', 'frames', 'obs_dev', 'final_obs_dev', 'restarted_dev', 'rewards_dev', 'info_dev', 'done_dev', 'frames_dev', 'shaped_dev', 'out_dtype', 'first_rows'}
    for name in ('mate_engine_enable_frame_fragments', 'mate_engine_frame_fragment'):
        assert name in _native.EXPORTED_SYMBOLS and re.search(r'\bint\s+' + name + r'\s*\(', header)
    lib = _native.load()
    assert all(hasattr(lib, name) for name in ('mate_engine_enable_frame_fragments', 'mate_engine_frame_fragment'))
    assert lib.mate_engine_enable_frame_fragments(None, None) == -1      # MATE_EINVAL: a null engine, no GPU touched
    from mate_amd import build
    names = {os.path.basename(d) for d in build.DEPS}
    assert {'frame_rows.hpp', 'frame_host.inc'} <= names
    with open(os.path.join(ROOT, 'mate_amd', 'csrc', 'frame_rows.hpp')) as fh:
        assert 'fragment_frame_kernel' in fh.read()
    with open(os.path.join(ROOT, 'mate_amd', 'lib', 'kernel_resources_opponents.json')) as fh:
        import json
        mine = {k: r for k, r in json.load(fh).items() if 'fragment_frame_kernel' in k}
    assert len(mine) == 2
    for r in mine.values():
        assert r['VGPRs'] <= 128 and r['Occupancy'] >= 4 and r['SGPRs Spill'] == 0 and r['VGPRs Spill'] == 0 and r['ScratchSize'] == 0 and r['Dynamic Stack'] == 'False'


def test_per_frame_arguments_accept_what_the_fused_fragment_refuses():
    from mate_amd.config import read_config
    from mate_amd.environment import fragment_arguments
    cfg = read_config('MATE-4v8-9.yaml')
    spec = fragment_arguments(cfg, 5, 'camera', target_agent='heuristic', per_frame=True)
    assert spec == {'frame_skip': 5, 'learner': 'camera', 'shaping': None, 'per_frame': True}
    assert fragment_arguments(cfg, 5, 'target', camera_agent='heuristic', per_frame=True)['per_frame']
    for key in REFUSED:
        for team in ('camera', 'target'):
            from mate_amd.engine import reward_term_keys
            if key in reward_term_keys(team):
                spec = fragment_arguments(cfg, 3, team, per_frame=True, **{team + '_reward_shaping': ({key: 0.5}, 'none')})
                assert spec['shaping'] == ({key: 0.5}, 'none')
    # what stays refused with per_frame: the other team's shaping, unknown keys, the row modes, selection, no frame_skip
    for bad in (dict(learner='camera', target_reward_shaping=({'coverage_rate': 1.0}, 'none')), dict(learner='camera', camera_reward_shaping=({'no_such': 1.0}, 'none')),
                dict(learner='camera', enhanced_observation='camera'), dict(learner='camera', camera_selection='multi'), dict(learner=None)):
        with pytest.raises(AssertionError):
            fragment_arguments(cfg, 5, per_frame=True, **bad)
    with pytest.raises(AssertionError, match='per_frame'):
        fragment_arguments(cfg, None, None, per_frame=True)


def test_without_per_frame_every_refusal_stays():
    from mate_amd.config import read_config
    from mate_amd.environment import fragment_arguments
    cfg = read_config('MATE-4v8-9.yaml')
    assert fragment_arguments(cfg, 5, 'camera') == {'frame_skip': 5, 'learner': 'camera', 'shaping': None}
    with pytest.raises(AssertionError, match='step per frame instead'):
        fragment_arguments(cfg, 5, 'camera', target_agent='heuristic')
    with pytest.raises(AssertionError, match='step per frame instead'):
        fragment_arguments(cfg, 5, 'target', camera_agent='heuristic')
    for key in REFUSED:
        with pytest.raises(AssertionError, match=key):
            fragment_arguments(cfg, 5, 'target' if key != 'soft_coverage_score' else 'camera',
                               **{('target' if key != 'soft_coverage_score' else 'camera') + '_reward_shaping': ({key: 1.0}, 'none')})
