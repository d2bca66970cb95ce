"""The communication arrows without a GPU: tests/render_comm_ref.py's restatement of RenderCommunication -- the trace rule and the
callback's lines -- against the reference's own recordings (tests/golden/render_comm_*.npz, tests/golden/make_render_comm_golden.py), known answers of the
dashed-line rule, the rim condition the device comparison rests on, the C ABI, its binding, the docstrings and the new unit's resource record.  The known
answers pin tests/render_comm_ref.py, the yardstick the device is then held to in tests/test_gpu_render_comm.py and tests/test_gpu_comm_trace.py."""
import json
import os
import re

import numpy as np
import pytest

import render_comm_ref as RC
import render_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def load(name):
    return RC.load_recording(os.path.join(GOLDEN, 'render_comm_%s.npz' % name))


@pytest.fixture(scope='module', params=RC.SCENES)
def recording(request):
    return (request.param,) + load(request.param)


def matrices_of(fx):
    return fx['comm/camera'], fx['comm/target']


# ------------------------------------------------------------------ the recordings
def test_the_restated_list_is_the_recorded_one(recording):
    """Order, kinds, colours, widths, stipples and counts exactly, vertices within 1e-9: the arrows sit behind the static geoms, ahead of the first sector."""
    name, recorded, scene, fx = recording
    mine = RC.display_list(scene, matrices_of(fx), int(fx['comm/duration']))
    assert int(fx['num_images']) == 4
    assert [p['kind'] for p in mine] == [p['kind'] for p in recorded]
    assert [len(p['v']) for p in mine] == [len(p['v']) for p in recorded]
    static = 5 + len(scene['obs_xyr'])
    lines = [i for i, p in enumerate(recorded) if p['kind'] == 'line']
    assert lines == list(range(static, static + len(lines))) and len(lines) > 0, name
    for i, (a, b) in enumerate(zip(mine, recorded)):
        assert tuple(a['rgba']) == tuple(b['rgba']), (name, i, a['rgba'], b['rgba'])
        if b['kind'] == 'line':
            assert (a['width'], a['stipple']) == (b['width'], b['stipple']) == (2.5, 0x0F0F), (name, i)
        else:
            assert a['width'] == (b['width'] if b['kind'] == 'polyline' else 0.0), (name, i)
        assert np.abs(a['v'] - b['v']).max() <= 1e-9, (name, i, np.abs(a['v'] - b['v']).max())


def test_the_trace_rule_reproduces_the_recorded_matrices(recording):
    name, _, _, fx = recording
    duration = int(fx['comm/duration'])
    for team in ('camera', 'target'):
        edges = fx['edges/' + team]
        remaining = np.zeros(edges.shape[1:], dtype=np.uint8)
        for step in range(len(edges)):
            remaining = RC.trace_step(remaining, edges[step], duration)
        assert np.array_equal(remaining, fx['comm/' + team]), (name, team)
    assert len(fx['edges/camera']) == RC.RECIPES[name][1]


def test_the_scenes_show_what_they_were_chosen_for():
    def arrows(name):
        prims, _, fx = load(name)
        lines = [p for p in prims if p['kind'] == 'line']
        return lines, fx
    for name in ('4v8-9_a', '4v8-9_b'):
        lines, fx = arrows(name)
        assert all(p['rgba'][:3] == (0.0, 0.0, 1.0) for p in lines) and str(fx['config_file']) == 'MATE-4v8-9.yaml'
    _, fx = arrows('4v8-9_a')
    m = fx['comm/camera']
    assert ((m > 0) & (m.T > 0)).any()                                                  # bidirectional pairs: two lines each
    lines, fx = arrows('4v8-9_b')
    m = fx['comm/camera']
    assert ((m > 0) & ~(m.T > 0)).any() and len({p['rgba'][3] for p in lines}) >= 4     # unidirectional pairs (three lines), several alpha values
    lines, fx = arrows('8v8-9')
    assert str(fx['config_file']) == 'MATE-8v8-9.yaml' and len(lines) > 0
    lines, fx = arrows('duration3')
    assert int(fx['comm/duration']) == 3 and {p['rgba'][3] for p in lines} <= {min(1.0, 1.2 * k / 3) for k in (1, 2, 3)}
    lines, fx = arrows('nocamera')
    assert not fx['comm/camera'].any() and fx['comm/target'].any() and all(p['rgba'][:3] == (1.0, 0.0, 0.0) for p in lines)
    m = fx['comm/target']
    assert ((m > 0) & (m.T > 0) & ~np.eye(len(m), dtype=bool)).any() and ((m > 0) & ~(m.T > 0)).any() and np.diag(m).any()      # both kinds, and a sender's own copy: no arrow


def test_rim_pixels_are_rare_at_every_size_the_device_is_compared_at(recording):
    """3.20's condition with the dash switches added: at most 0.1 % of a frame at every (scene, size) the device tests draw."""
    name, recorded, _, _ = recording
    for size in RC.SIZES[name]:
        share = RC.rim(recorded, size).mean()
        assert share <= 1e-3, (name, size, share)


# ------------------------------------------------------------------ known answers
def line(a, b, alpha=1.0):
    return {'kind': 'line', 'v': np.array([a, b], dtype=np.float64), 'rgba': (0.0, 0.0, 1.0, alpha), 'width': RC.STROKE, 'stipple': RC.STIPPLE}


def test_the_trace_rule():
    remaining = np.array([[0, 5], [1, 20]], dtype=np.uint8)
    after = RC.trace_step(remaining, np.array([[0, 0], [0, 1]]), 20)
    assert after.tolist() == [[0, 4], [0, 20]] and after.dtype == np.uint8
    assert RC.trace_step(after, np.array([[3, 0], [0, 0]]), 7).tolist() == [[7, 3], [0, 19]]


def test_a_horizontal_line_is_on_in_the_columns_whose_count_from_the_first_vertex_is_below_four_mod_eight():
    size = 200                                                          # pitch 10.5; centres at -1050 + 10.5 (c + 0.5)
    p = R.pitch_of(size)
    row, first = 100, 20
    y, x0 = R.centres(size)[1][row], R.centres(size)[0][first] - 0.25 * p      # along a row of centres, from a quarter pitch left of a centre: u = k + 0.25 in column first + k
    x1 = x0 + 40.5 * p
    covered = RC.cover_line(line((x0, y), (x1, y)), size)
    inside = slice(first, first + 41)
    on = [k for k in range(41) if k % 8 < 4]
    assert list(np.flatnonzero(covered[row, inside])) == on
    assert list(np.flatnonzero(covered[row - 1, inside])) == on and list(np.flatnonzero(covered[row + 1, inside])) == on      # 1.25 pitches: the rows one above and below
    assert not covered[row - 2].any() and not covered[row + 2].any()
    # the count starts at the FIRST vertex: the same segment drawn the other way round is on from its other end
    back = RC.cover_line(line((x1, y), (x0, y)), size)
    assert list(np.flatnonzero(back[row, inside])) == [k for k in range(41) if (40 - k) % 8 < 4]
    # beyond the ends the projection is clamped: the cap of the first vertex is on (u = 0), that of the last has its phase (u = 40: on)
    assert covered[row, first - 1] and covered[row, first + 41] and not covered[row, first - 2]


def test_a_steep_line_counts_along_y():
    size = 200
    p = R.pitch_of(size)
    xs, ys = R.centres(size)
    col, top = 60, 30
    covered = RC.cover_line(line((xs[col], ys[top] + 0.25 * p), (xs[col] + 3 * p, ys[top] - 30.25 * p)), size)      # ~30 rows down, 3 columns right: the major axis is y
    for k in range(31):
        c = col + int(round(3 * k / 30))
        assert covered[top + k, c] == (k % 8 < 4), k
    flat = RC.cover_line(line((xs[col] - 0.25 * p, ys[top]), (xs[col] + 30.25 * p, ys[top] - 3 * p)), size)      # the same slope the other way: along x
    for k in range(31):
        assert flat[top + int(round(3 * k / 30)), col + k] == (k % 8 < 4), k


def test_lines_blend_once_each_in_list_order():
    size = 64
    y = R.centres(size)[1][32]
    a, b = line((-500.0, y), (500.0, y), 0.5), line((-500.0, y), (500.0, y), 0.25)
    b['rgba'] = (1.0, 0.0, 0.0, 0.25)
    image = RC.rasterise([a, b], size)
    c = np.ones(3, dtype=np.float32)
    for prim in (a, b):
        al = np.float32(prim['rgba'][3])
        c = np.array(prim['rgba'][:3], dtype=np.float32) * al + c * (np.float32(1.0) - al)
    col = int(np.flatnonzero(RC.cover_line(a, size)[32])[0])
    assert tuple(image[32, col]) == tuple(int(v) for v in np.floor(np.float32(255.0) * c + np.float32(0.5)))
    assert tuple(image[0, 0]) == (255, 255, 255)


def test_draw_arrow_known_answers():
    one = RC.draw_arrow((0.0, 0.0), (100.0, 0.0), (0.0, 0.0, 1.0, 1.0), False)
    assert len(one) == 3 and np.allclose(one[0]['v'], [[10.0, 0.0], [90.0, 0.0]])              # shortened to 0.9 of a short vector
    assert np.allclose(one[1]['v'], [[90.0 - 3.6, 1.35], [90.0, 0.0]]) and np.allclose(one[2]['v'], [[90.0 - 3.6, -1.35], [90.0, 0.0]])
    both = RC.draw_arrow((0.0, 0.0), (1000.0, 0.0), (0.0, 0.0, 1.0, 1.0), True)
    assert len(both) == 2 and np.allclose(both[0]['v'], [[50.0, 10.0], [950.0, 10.0]])         # by 50 at either end of a long one, 10 sideways
    head = both[1]['v'][1] - both[1]['v'][0]
    assert np.allclose(head, [38.0, -14.25]) and np.hypot(*head) < 50.0
    far = RC.draw_arrow((0.0, 0.0), (2000.0, 0.0), (0.0, 0.0, 1.0, 1.0), False)
    assert np.isclose(np.hypot(*(far[1]['v'][1] - far[1]['v'][0])), 50.0)                      # the head's clamp
    assert RC.draw_arrow((3.0, 4.0), (3.0, 4.0), (0.0, 0.0, 1.0, 1.0), False) == []


# ------------------------------------------------------------------ the ABI, its binding, the docstrings, the unit's record
def test_header_binding_and_docstrings_agree():
    with open(os.path.join(ROOT, 'include', 'mate_engine.h')) as fh:
        header = fh.read()
    assert re.search(r'#define\s+MATE_ABI_VERSION\s+1\b', header)
    assert re.search(r'int\s+mate_engine_enable_comm_trace\s*\(\s*mate_engine\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)\s*;', header)
    assert re.search(r'int\s+mate_engine_comm_trace\s*\(\s*mate_engine\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*uint8_t\s*\*\*\s*\w+\s*,\s*int32_t\s*\*\*\s*\w+\s*\)\s*;', header)
    assert re.search(r'int\s+mate_engine_set_comm_trace\s*\(\s*mate_engine\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*const\s+uint8_t\s*\*\s*\w+\s*\)\s*;', header)
    from mate_amd import _native
    from mate_amd.engine import Engine, EngineGroups
    from mate_amd.environment import BatchedMultiAgentTracking, MultiAgentTracking
    assert [len(_native.PROTOTYPES['mate_engine_' + name][1]) for name in ('enable_comm_trace', 'comm_trace', 'set_comm_trace', 'render')] == [3, 4, 3, 7]
    assert 'transparent channel' in Engine.enable_communication_trace.__doc__ and 'set_channel(team)' in Engine.enable_communication_trace.__doc__
    assert 'uint8' in Engine.communication_trace.__doc__ and callable(EngineGroups.enable_communication_trace) and callable(EngineGroups.communication_trace)
    assert callable(BatchedMultiAgentTracking.communication_trace) and 'message_buffers' in MultiAgentTracking.enable_render_communication.__doc__
    with open(os.path.join(ROOT, 'mate_amd', 'csrc', 'render_rows.hpp')) as fh:
        source = fh.read()
    chunk, words, pairs = (int(re.search(r'%s\s*=\s*(\d+)' % k, source).group(1)) for k in ('kRenderArrowChunk', 'kRenderArrowWords', 'kRenderMaxPairs'))
    # the largest shape (16 / 16 / 64) with the arrows' part still fits the LDS a launch has without opting in; every pair of it has a slot in the list
    assert pairs == 2 * 16 * 16 and chunk <= 256 and 36160 + chunk * words * 8 + pairs * 2 + 16 <= 64 * 1024
    from mate_amd.evaluate import build_parser
    args = build_parser().parse_args(['--save-frames', 'out', '--render-communication'])
    assert args.render_communication == 20 and build_parser().parse_args(['--render-communication', '5']).render_communication == 5
    assert build_parser().parse_args([]).render_communication is None


def test_the_units_resource_record():
    from mate_amd import build
    lib = os.path.join(ROOT, 'mate_amd', 'lib')
    assert [(unit[1], unit[3]) for unit in build.TRACE_UNITS] == [('trace_kernels.hip', 'trace_resources.json')]
    path = os.path.join(lib, 'trace_resources.json')
    assert os.path.exists(path), 'run __graft_entry__.build() first'
    with open(path) as fh:
        record = json.load(fh)
    assert any('comm_trace_kernel' in name for name in record)
    for name, r in record.items():
        assert r['ScratchSize'] == 0 and r['Dynamic Stack'] == 'False' and r['SGPRs Spill'] == 0 and r['VGPRs Spill'] == 0, (name, r)
        assert r['VGPRs'] <= 128 and r['Occupancy'] >= 4, (name, r)
    for other in os.listdir(lib):
        if other != 'trace_resources.json' and other.endswith('.json') and other != 'build_stamp.json':
            with open(os.path.join(lib, other)) as fh:
                assert not any('comm_trace_kernel' in name for name in json.load(fh)), other
    for source in ('trace_rows.hpp', 'trace_kernels.hip', 'trace_host.inc'):
        assert os.path.join(ROOT, 'mate_amd', 'csrc', source) in build.DEPS
