"""The inputs of the entity-count edge matrix (tests/shape_edges.py, tests/test_gpu_shape_edges.py) exercise the edges they are
named for: with the oracle alone, under the same seed, batch and step count as the GPU test, the targets of every case run
into camera bodies -- past the 64th circle where the case is about that -- often enough that a kernel which skipped those
circles could not agree with the oracle."""
import pytest

import shape_edges as S

MIN_EVENTS = 100
MIN_STRADDLING_FRAMES = 20


@pytest.mark.parametrize('case', S.CASES, ids=S.case_id)
def test_edge_scenarios_collide_with_the_circles_they_are_about(case, oracle_lib):
    nc, nt, no = case.shape
    counts = S.count_events(oracle_lib, case)
    print(S.case_id(case), counts)
    if nc:
        assert counts['camera'] >= MIN_EVENTS, (S.case_id(case), counts)
    else:       # no cameras: the circles are obstacles, the last one first (shape_edges.scenario)
        assert counts['obstacle'] >= MIN_EVENTS, (S.case_id(case), counts)
    if nc + no > 64:
        assert counts['camera_past_64'] >= MIN_EVENTS, (S.case_id(case), counts)
    assert counts['colliding'] >= MIN_EVENTS, (S.case_id(case), counts)


@pytest.mark.parametrize('name', ['7v5-3', '16v15-3', '5v7-0'])
def test_attached_scenarios_fill_their_straddling_rows(name, oracle_lib):
    """The cases of ATTACHED_CASES whose camera_target_view_mask rows cross a 32-bit word: under the random policy every such row has a
    seen target on each side of the boundary at once in at least MIN_STRADDLING_FRAMES (environment, step) frames -- a row taken from
    its first word alone could not agree with the row."""
    case = S.attached_case(name)
    nc, nt, _ = case.shape
    rows = S.straddling_rows(nc, nt)
    assert rows == {'7v5-3': {6: 2}, '16v15-3': {2: 2, 4: 4, 6: 6, 8: 8, 10: 10, 12: 12, 14: 14}, '5v7-0': {4: 4}}[name]
    frames = S.count_straddling_frames(oracle_lib, case)
    print(name, 'frames per straddling row', frames)
    assert set(frames) == set(rows) and min(frames.values()) >= MIN_STRADDLING_FRAMES, (name, frames)


def test_attached_scenarios_have_the_shapes_they_claim():
    """The arithmetic the attached cases stand on: view bits and words, odd state-row widths, and no straddle where Nt divides 32."""
    assert [c.shape for c in S.ATTACHED_CASES] == [(7, 5, 3), (16, 15, 3), (5, 7, 0), (16, 16, 9), (0, 5, 64), (16, 16, 64)]
    assert all(S.straddling_rows(nc, nt) == {} for nc in (1, 4, 16) for nt in (1, 2, 4, 8, 16))
    assert S.straddling_rows(3, 5) == {} and 16 * 15 == 240 and (14 * 15 + 14) // 32 == 7      # row 14 ends in the eighth word of eight
    state_dim = lambda nc, nt, no: 13 + 9 * nc + 14 * nt + 3 * no + 2 * nt + 16  # noqa: E731  (csrc/state_rows.hpp state_dim_of)
    assert state_dim(7, 5, 3) == 181 and state_dim(16, 16, 64) == 621
    for case in S.ATTACHED_CASES:
        cfg = S.case_scenario(case)
        got = tuple(len(cfg.get(k, {}).get('location_random_range', [])) for k in ('camera', 'target', 'obstacle'))
        assert got == case.shape and 8 <= case.n <= 48
        if case.target_box is not None:
            assert all(box == [-case.target_box, case.target_box] * 2 for box in cfg['target']['location_random_range'])
    view = __import__('numpy').zeros((2, 7, 5), dtype=bool)
    view[0, 6, [1, 2]] = True      # bits 31 and 32: one on each side
    view[1, 6, [2, 3]] = True      # bits 32 and 33: both in the upper word
    assert S.straddling_frames(view) == {6: 1}


def test_edge_scenarios_have_the_shapes_and_thresholds_they_claim():
    """The arithmetic the cases are chosen by, so that a change of a kernel threshold shows up here as a case to move."""
    shapes = [c.shape for c in S.CASES]
    assert shapes == [(1, 2, 64), (16, 16, 64), (16, 3, 48), (0, 5, 64), (0, 6, 64), (4, 16, 16), (4, 16, 17), (3, 5, 7), (9, 2, 0)]
    nk = {s: s[0] + s[2] for s in shapes}
    assert nk[(1, 2, 64)] == 65 and nk[(16, 16, 64)] == 80 and nk[(16, 3, 48)] == nk[(0, 5, 64)] == nk[(0, 6, 64)] == 64
    assert 5 * nk[(0, 5, 64)] == 320 and 6 * nk[(0, 6, 64)] > 320 and 16 * nk[(4, 16, 16)] == 320 and 16 * nk[(4, 16, 17)] == 336
    for case in S.CASES + S.GREEDY_CASES:
        cfg = S.scenario(case.shape)
        got = tuple(len(cfg.get(k, {}).get('location_random_range', [])) for k in ('camera', 'target', 'obstacle'))
        assert got == case.shape and 8 <= case.n <= 48 and 30 <= case.steps <= 60


def test_reference_trace_past_64_circles_walks_into_a_camera():
    """tests/golden/trace_2v3-64_random_s8.npz (the reference itself on 2 cameras behind 64 obstacles, replayed on the oracle by
    test_oracle_golden.py and on the engine by test_gpu_parity.py): its targets do collide with camera 1, circle 65 of their walk."""
    import numpy as np
    import golden_util as G
    fx = G.load('trace_2v3-64_random_s8.npz')
    assert (int(fx['num_cameras']), int(fx['num_targets']), int(fx['num_obstacles'])) == (2, 3, 64)
    pos = np.concatenate([fx['reset/tgt_xy'][None], fx['step/tgt_xy'][:-1]])
    act, limit = fx['step/tgt_act'], fx['static/tgt_step_size']
    norm = np.hypot(act[..., 0], act[..., 1])
    dest = pos + act * np.where(norm > limit, limit / np.maximum(norm, 1e-300), 1.0)[..., None]
    inside = np.hypot(*np.moveaxis(dest[:, :, None, :] - fx['static/cam_xy'][None, None], -1, 0)) < fx['static/cam_radius']
    hits = (fx['step/tgt_colliding'].astype(bool)[:, :, None] & inside).sum(axis=(0, 1))
    assert hits[1] >= 20, hits.tolist()
