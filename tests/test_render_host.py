"""The off-screen render without a GPU: tests/render_ref.py's restatement of the display list against the reference's own recorded
lists (tests/golden/render_*.npz, tests/golden/make_render_golden.py), known answers of the rasteriser's rules, the rim condition the device comparison
rests on, the C ABI, its binding and the kernel's resource record, the evaluate tool's PNG writer.  The known answers (the fan rule, the blend order, the
polyline band, the row orientation) pin tests/render_ref.py, the yardstick the device is then held to in tests/test_gpu_render.py: they say nothing about
the kernel by themselves."""
import json
import os
import re
import struct
import zlib

import numpy as np
import pytest

import render_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
# every (scene, size) tests/test_gpu_render.py draws and compares
SIZES = {scene: (64, 200) for scene in R.SCENES}
SIZES['4v8-9_random'] = (64, 200, 800)
SIZES['2v4-0'] = (64, 72, 200)
F = np.float32


@pytest.fixture(scope='module', params=R.SCENES)
def recording(request):
    return (request.param,) + R.load_recording(os.path.join(GOLDEN, 'render_%s.npz' % request.param))


def test_the_restated_list_is_the_recorded_one(recording):
    name, recorded, scene, fx = recording
    mine = R.display_list(scene)
    assert int(fx['num_images']) == 4                                  # the warehouse icons: recorded, not drawn
    assert [p['kind'] for p in mine] == [p['kind'] for p in recorded]
    assert [len(p['v']) for p in mine] == [len(p['v']) for p in recorded]
    for i, (a, b) in enumerate(zip(mine, recorded)):
        assert tuple(a['rgba']) == tuple(b['rgba']), (name, i)
        assert a['width'] == (b['width'] if b['kind'] == 'polyline' else 0.0), (name, i)
        assert np.abs(a['v'] - b['v']).max() <= 1e-9, (name, i, np.abs(a['v'] - b['v']).max())


def test_the_scenes_show_what_they_were_chosen_for():
    load = lambda name: R.load_recording(os.path.join(GOLDEN, 'render_%s.npz' % name))      # noqa: E731
    colours = lambda prims: {p['rgba'] for p in prims}      # noqa: E731
    prims, scene, _ = load('4v8-9_random')
    assert {(0.0, 0.6, 0.0, 0.25), (0.6, 0.6, 0.0, 0.25)} <= colours(prims)                  # both polygon colours
    assert max(len(p['v']) for p in prims) > 100                                                # occlusion notches: knots between the integer degrees
    prims, scene, _ = load('8v8-9_greedy')
    assert (1.0, 1.0, 0.0, 1.0) in colours(prims) and (0.6, 0.2, 0.1, 1.0) in colours(prims)  # tracked markers, a perceived camera
    prims, scene, _ = load('2v4-0')
    assert len(scene['obs_xyr']) == 0
    prims, scene, _ = load('fewcargo')
    assert (1.0, 1.0, 1.0, 0.66) in colours(prims) and {p['rgba'][3] for p in prims[1:5]} == {0.3, 0.6}
    prims, scene, _ = load('seam180')
    left = R.normalize_angle(scene['cam_phi'][0] - 90.0)
    assert scene['cam_theta'][0] == 180.0 and left + 180.0 > 180.0                              # boundary_between's angle_right > 180 branch
    prims, scene, _ = load('navigation')
    assert len(scene['cam_phi']) == 0


def test_rim_pixels_are_rare_at_every_size_the_device_is_compared_at(recording):
    name, recorded, scene, fx = recording
    for size in SIZES[name]:
        share = R.rim(recorded, size).mean()
        assert share <= 1e-3, (name, size, share)


# ------------------------------------------------------------------ known answers
CONCAVE = 50.0 * np.array([(0.0, 0.0), (10.0, 0.0), (10.0, 10.0), (5.0, 2.0), (0.0, 10.0)])      # vertex 0 does not see the notch above vertex 3


def pixel_of(x, y, size):
    p = R.pitch_of(size)
    return int(np.floor((R.BOUND - y) / p)), int(np.floor((x + R.BOUND) / p))


def test_a_polygon_with_more_than_four_vertices_is_the_union_of_its_fan():
    size = 210                                                          # pitch 10: centres at -1045 + 10 c
    covered = R.cover_polygon(CONCAVE, size)
    assert covered[pixel_of(255.0, 205.0, size)]                        # in the notch of the outline, inside the fan triangle (v0, v1, v2)
    assert not covered[pixel_of(105.0, 405.0, size)] and not covered[pixel_of(-5.0, 5.0, size)]
    assert covered[pixel_of(255.0, 155.0, size)]                        # inside two fan triangles ...
    image = R.rasterise([R.polygon(CONCAVE, (0.0, 0.0, 0.0), 0.5)], size)
    assert tuple(image[pixel_of(255.0, 155.0, size)]) == (128, 128, 128)      # ... and blended once: floor(255 * 0.5 + 0.5)
    square = R.cover_polygon(100.0 * R.SQUARE, size)
    assert square.sum() == 20 * 20


def test_blending_is_in_list_order_in_f32_and_quantised_once():
    size = 64
    a, b = (0.6, 0.6, 0.0, 0.25), (0.0, 0.6, 0.8, 0.1)
    first = R.rasterise([R.polygon(500.0 * R.SQUARE, a[:3], a[3]), R.polygon(500.0 * R.SQUARE, b[:3], b[3])], size)
    second = R.rasterise([R.polygon(500.0 * R.SQUARE, b[:3], b[3]), R.polygon(500.0 * R.SQUARE, a[:3], a[3])], size)
    pixel = pixel_of(0.0, 0.0, size)

    def expect(order):
        c = np.ones(3, dtype=F)
        for rgba in order:
            c = np.array(rgba[:3], dtype=F) * F(rgba[3]) + c * (F(1.0) - F(rgba[3]))
        return tuple(int(v) for v in np.floor(F(255.0) * c + F(0.5)))
    assert tuple(first[pixel]) == expect((a, b)) and tuple(second[pixel]) == expect((b, a)) and expect((a, b)) != expect((b, a))
    assert tuple(first[0, 0]) == (255, 255, 255)                        # the background is white


def test_a_polyline_covers_the_centres_within_half_its_width():
    size = 200                                                          # pitch 10.5: |x + 1000| <= 15.75 holds for columns 3, 4, 5
    margin = {'kind': 'polyline', 'v': 1000.0 * R.SQUARE, 'rgba': (0.0, 0.0, 0.0, 1.0), 'width': 3.0}
    image = R.rasterise([margin], size)
    row = image[size // 2, :, 0]
    assert list(np.flatnonzero(row == 0)) == [3, 4, 5, 194, 195, 196]
    assert list(np.flatnonzero(image[:, size // 2, 0] == 0)) == [3, 4, 5, 194, 195, 196]


def test_row_zero_is_the_top():
    size = 64
    image = R.rasterise([R.polygon(R.placed(100.0 * R.SQUARE, (-800.0, 700.0)), (1.0, 0.0, 0.0))], size)
    rows, cols = np.nonzero(image[:, :, 1] == 0)
    assert rows.max() < size // 4 and cols.max() < size // 4 and len(rows) > 0
    xs, ys = R.centres(size)
    assert ys[0] > ys[-1] and xs[0] < xs[-1] and xs[0] == -R.BOUND + R.pitch_of(size) / 2


# ------------------------------------------------------------------ the ABI, its binding, the kernel's record
def test_header_binding_and_kernel_constants_agree():
    with open(os.path.join(ROOT, 'include', 'mate_engine.h')) as fh:
        header = fh.read()
    assert re.search(r'#define\s+MATE_ABI_VERSION\s+1\b', header)
    assert re.search(r'int\s+mate_engine_render\s*\(\s*mate_engine\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*,\s*int32_t\s+\w+\s*,'
                     r'\s*const\s+double\s*\*\s*\w+\s*,\s*uint8_t\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;', header)
    lo, hi = (int(re.search(r'#define\s+MATE_RENDER_%s_SIZE\s+(\d+)' % k, header).group(1)) for k in ('MIN', 'MAX'))
    from mate_amd import _native
    from mate_amd.engine import Engine
    assert len(_native.PROTOTYPES['mate_engine_render'][1]) == 7 and len(_native.PROTOTYPES['mate_engine_keep_masks'][1]) == 1
    assert re.search(r'int\s+mate_engine_keep_masks\s*\(\s*mate_engine\s*\*\s*\w+\s*\)\s*;', header)
    assert Engine.RENDER_SIZES == (lo, hi) == (16, 4096)
    with open(os.path.join(ROOT, 'mate_amd', 'csrc', 'render_rows.hpp')) as fh:
        source = fh.read()
    assert re.search(r'kRenderMinSize\s*=\s*%d\s*,\s*kRenderMaxSize\s*=\s*%d\b' % (lo, hi), source)
    words, cam, slots_max = (int(re.search(r'%s\s*=\s*(\d+)' % k, source).group(1)) for k in ('kRenderPrimWords', 'kRenderCamWords', 'kRenderMaxSlots'))
    # the largest shape the engine takes (16 cameras, 16 targets, 64 obstacles) fits the slot table and the LDS a launch has without opting in
    slots = 5 + 64 + 4 * 16 + 3 * 16
    assert slots <= slots_max and (slots * words + 16 * cam + 2 * 87) * 8 + 2 * slots_max + 768 + 96 <= 64 * 1024
    assert (words * 8) % 16 == 0 and (cam * 8) % 16 == 0              # every part of the dynamic LDS starts on a 16-byte boundary


def test_the_kernels_resource_record():
    from mate_amd import build
    lib = os.path.join(ROOT, 'mate_amd', 'lib')
    assert [(unit[1], unit[3]) for unit in build.LATER_UNITS] == [('render_kernels.hip', 'render_resources.json')]
    path = os.path.join(lib, 'render_resources.json')
    assert os.path.exists(path), 'run __graft_entry__.build() first'
    with open(path) as fh:
        record = json.load(fh)
    assert len(record) == 2 and all('render_kernel' in name for name in record)
    for name, r in record.items():
        assert r['ScratchSize'] == 0 and r['Dynamic Stack'] == 'False' and r['SGPRs Spill'] == 0 and r['VGPRs Spill'] == 0, (name, r)
        assert r['VGPRs'] <= 128 and r['Occupancy'] >= 4, (name, r)
    for other in os.listdir(lib):
        if other.startswith('kernel_resources') and other.endswith('.json'):
            with open(os.path.join(lib, other)) as fh:
                assert not any('render_kernel' in name for name in json.load(fh)), other
    assert os.path.join(ROOT, 'mate_amd', 'csrc', 'render_rows.hpp') in build.DEPS and os.path.join(ROOT, 'mate_amd', 'csrc', 'render_kernels.hip') in build.DEPS


# ------------------------------------------------------------------ the evaluate tool's writer
def test_write_png_round_trip(tmp_path):
    from mate_amd.evaluate import FrameSaver, build_parser, write_png
    image = np.random.RandomState(0).randint(0, 256, size=(17, 23, 3)).astype(np.uint8)
    path = str(tmp_path / 'x.png')
    write_png(path, image)
    with open(path, 'rb') as fh:
        data = fh.read()
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    chunks, at = [], 8
    while at < len(data):
        n, = struct.unpack('>I', data[at:at + 4])
        tag, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert struct.unpack('>I', data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        chunks.append((tag, body))
        at += 12 + n
    assert [tag for tag, _ in chunks] == [b'IHDR', b'IDAT', b'IEND']
    assert struct.unpack('>IIBBBBB', chunks[0][1]) == (23, 17, 8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(17, 1 + 23 * 3)
    assert not rows[:, 0].any() and np.array_equal(rows[:, 1:].reshape(17, 23, 3), image)
    saver = FrameSaver(str(tmp_path / 'frames'), size=16, every=2)
    for _ in range(5):
        saver(lambda size: np.zeros((size, size, 3), dtype=np.uint8))
    assert [os.path.basename(p) for p in saver.written] == ['frame_000000.png', 'frame_000002.png', 'frame_000004.png'] and all(os.path.exists(p) for p in saver.written)
    args = build_parser().parse_args(['--save-frames', 'out', '--frame-size', '200', '--frame-every', '3'])
    assert (args.save_frames, args.frame_size, args.frame_every) == ('out', 200, 3)
