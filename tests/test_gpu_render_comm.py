"""The communication arrows on the device (csrc/render_rows.hpp) against tests/render_comm_ref.py: the reference's own recorded display
lists with RenderCommunication's lines (tests/golden/render_comm_*.npz) rasterised in NumPy, pixel for pixel outside the rim, from a planted trace; an empty
and a stale trace; indices; observation types; the closed loop from the engine's own trace; the two environment classes; the evaluate tool."""
import functools
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import render_comm_ref as RC
import render_ref as R
from test_gpu_render import IMPORT_KEYS, _same_outside_the_rim
from test_render_host import GOLDEN

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _recording(name):
    return RC.load_recording(os.path.join(GOLDEN, 'render_comm_%s.npz' % name))


@functools.lru_cache(maxsize=None)
def _expected(name, size):
    """(image, rim) of a recording at a size: computed once, shared, never written to."""
    prims, _, _ = _recording(name)
    image, rim = RC.rasterise(prims, size), RC.rim(prims, size)
    image.setflags(write=False)
    rim.setflags(write=False)
    return image, rim


@functools.lru_cache(maxsize=None)
def _planted(name, num_envs=1, obs_dtype=torch.float32, trace=True):
    """An engine whose every environment holds the recording's state, knots, view masks and -- `trace` -- the wrapper's two matrices."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    _, scene, fx = _recording(name)
    eng = Engine(read_config(str(fx['config_file']), max_episode_steps=int(fx['max_episode_steps'])), num_envs, seed=0, obs_dtype=obs_dtype)
    eng.enable_policies()
    s = {k: scene[k] for k in ('cam_phi', 'cam_theta', 'tgt_capacity', 'tgt_goals', 'bounties', 'remaining_cargoes', 'awaiting_cargo_counts')}
    s.update(cam_x=scene['cam_xy'][:, 0], cam_y=scene['cam_xy'][:, 1], tgt_x=scene['tgt_xy'][:, 0], tgt_y=scene['tgt_xy'][:, 1],
             obs_x=scene['obs_xyr'][:, 0], obs_y=scene['obs_xyr'][:, 1], obs_radius=scene['obs_xyr'][:, 2])
    s.update({k: fx['import/' + k] for k in IMPORT_KEYS})
    fields = {k: np.broadcast_to(np.asarray(v, dtype=np.float64), (num_envs,) + np.shape(v)) for k, v in s.items()}
    fields.update(tick=np.zeros(num_envs), episode=np.ones(num_envs), done=np.zeros(num_envs))
    eng.import_state(torch.zeros((num_envs, eng.layout.export_width), dtype=torch.float64))
    eng.load_state_dict(fields)
    for c, (phis, rhos) in enumerate(scene['knots']):
        for e in range(num_envs):
            eng.lut_write(e, c, phis, rhos)
    eng.observe()
    torch.cuda.synchronize()
    masks = eng.unpack_masks()
    for key in ('camera_target_view_mask', 'target_camera_view_mask'):
        assert np.array_equal(masks[key][0], scene[key].astype(bool).reshape(masks[key][0].shape)), (name, key)
    if trace:
        eng.enable_communication_trace(duration=int(fx['comm/duration']))
        for team, key in enumerate(('comm/camera', 'comm/target')):
            eng.set_communication_trace(team, np.broadcast_to(fx[key].astype(np.uint8), (num_envs,) + fx[key].shape))
    return eng


def _restated(eng, env, headings=None):
    """The list restated from the engine's own export and trace: the arrows of the teams whose tag is the environment's episode."""
    scene = R.scene_of_engine(eng, env, headings=headings)
    episode = int(eng.state_dict()['episode'][env])
    remaining = [eng.communication_trace(t)[env].cpu().numpy() if t in eng.trace_teams and int(eng.communication_trace_tags(t)[env]) == episode else None for t in (0, 1)]
    return RC.display_list(scene, remaining, eng.trace_duration)


# ------------------------------------------------------------------ 1. the recorded lists
@pytest.mark.parametrize('name,size', [(name, size) for name in RC.SCENES for size in RC.SIZES[name]])
def test_the_device_image_is_the_recorded_list_rasterised(name, size):
    """Every scene at 64, 200 and the tile-edge size 72, one at 800: the planted trace draws the RECORDED lines, at their recorded list position (a sector
    blends over them: at another position the pixels under the sectors differ)."""
    eng = _planted(name)
    prims, scene, _ = _recording(name)
    expected, rim = _expected(name, size)
    got = eng.render([0], size=size, headings=scene['target_orientations'][None])
    _same_outside_the_rim(got[0].cpu().numpy(), expected, rim, (name, size))
    lines = np.zeros((size, size), dtype=bool)
    for p in prims:
        if p['kind'] == 'line':
            lines |= RC.cover_line(p, size)
    assert lines.sum() > 0
    if size == 200:      # the yardstick itself: with the lines moved behind the sectors the expected image changes, so the comparison above can tell
        moved = [p for p in prims if p['kind'] != 'line'] + [p for p in prims if p['kind'] == 'line']
        assert (RC.rasterise(moved, size) != expected).any()


def test_an_empty_and_a_stale_trace_draw_the_frame_without_a_trace():
    name, size = '4v8-9_b', 72
    _, scene, fx = _recording(name)
    plain = _planted(name, trace=False).render([0], size=size, headings=scene['target_orientations'][None]).clone()
    eng = _planted(name, obs_dtype=torch.float64)      # (an engine of its own: this test rewrites its trace)
    headings = scene['target_orientations'][None]
    with_arrows = eng.render([0], size=size, headings=headings).clone()
    assert not torch.equal(with_arrows, plain)
    tags = [eng.communication_trace_tags(t) for t in (0, 1)]
    held = [t.clone() for t in tags]
    for t in tags:
        t.fill_(77)      # another episode's matrices: no arrow
    assert torch.equal(eng.render([0], size=size, headings=headings), plain)
    for t, h in zip(tags, held):
        t.copy_(h)
    assert torch.equal(eng.render([0], size=size, headings=headings), with_arrows)
    for team in (0, 1):
        eng.set_communication_trace(team, np.zeros_like(fx[('comm/camera', 'comm/target')[team]], dtype=np.uint8)[None])
    assert torch.equal(eng.render([0], size=size, headings=headings), plain)
    for team, key in enumerate(('comm/camera', 'comm/target')):      # back, for the f32 / f64 comparison below
        eng.set_communication_trace(team, fx[key].astype(np.uint8)[None])
    assert torch.equal(eng.render([0], size=size, headings=headings), _planted(name).render([0], size=size, headings=headings))      # f64 and f32 observation engines: the same bytes


def test_several_frames_with_unordered_indices():
    name, size = 'nocamera', 64
    _, scene, fx = _recording(name)
    eng = _planted(name, num_envs=5)
    rng = np.random.RandomState(1)
    traces = [(rng.rand(5, *fx[key].shape) < 0.3) * rng.randint(1, 21, size=(5,) + fx[key].shape) for key in ('comm/camera', 'comm/target')]
    traces[1][4] = 0      # one environment without a red arrow
    for team in (0, 1):
        eng.set_communication_trace(team, traces[team].astype(np.uint8))
    order = [3, 0, 3, 1, 4]
    frames = eng.render(order, size=size).cpu().numpy()
    assert np.array_equal(frames[0], frames[2]) and not np.array_equal(frames[0], frames[1])
    for k, env in enumerate(order):
        prims = _restated(eng, env)
        assert sum(p['kind'] == 'line' for p in prims) > 0
        _same_outside_the_rim(frames[k], RC.rasterise(prims, size), RC.rim(prims, size), ('k > 1', env))
        assert torch.equal(eng.render([env], size=size)[0].cpu(), torch.from_numpy(frames[k])), env
    for team, key in enumerate(('comm/camera', 'comm/target')):      # (the cached engine back as it was planted)
        eng.set_communication_trace(team, np.broadcast_to(fx[key].astype(np.uint8), (5,) + fx[key].shape))


# ------------------------------------------------------------------ 2. the closed loop
def test_forty_greedy_steps_then_a_render_against_the_restated_list():
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    from test_gpu_scripted import _plant_emptied_warehouses
    eng = Engine(read_config('MATE-4v8-9.yaml'), 6, seed=13)
    eng.enable_policies()
    eng.reset()
    _plant_emptied_warehouses(eng)
    eng.enable_communication_trace(duration=60)      # (the targets talk when a warehouse runs empty, early in the planted environments 0 and 3: their marks last)
    for _ in range(40):
        eng.step_greedy(auto_reset=1)
    torch.cuda.synchronize()
    assert eng.communication_trace('camera').any()
    envs, size = [0, 3, 5], 200
    frames = eng.render(envs, size=size).cpu().numpy()
    colours = set()
    for k, env in enumerate(envs):
        prims = _restated(eng, env)
        colours |= {p['rgba'][:3] for p in prims if p['kind'] == 'line'}
        _same_outside_the_rim(frames[k], RC.rasterise(prims, size), RC.rim(prims, size), ('closed loop', env))
    assert (0.0, 0.0, 1.0) in colours and ((1.0, 0.0, 0.0) in colours) == bool(eng.communication_trace('target')[envs].any())
    eng.reset()      # between a reset and the next step: the trace is another episode's, no arrow
    plain = [p for p in _restated(eng, 0)]
    assert not any(p['kind'] == 'line' for p in plain)
    _same_outside_the_rim(eng.render([0], size=64)[0].cpu().numpy(), RC.rasterise(plain, 64), RC.rim(plain, 64), 'behind a reset')


# ------------------------------------------------------------------ 3. the environment classes, the tool
def test_the_single_environment_class_keeps_the_wrappers_matrices_on_the_host():
    import mate_amd
    from mate_amd.utils import Message, Team
    env = mate_amd.MultiAgentTracking('MATE-4v8-9.yaml')
    env.enable_render_communication(duration=4)
    env.seed(3)
    env.reset()
    idle = (np.zeros((env.num_cameras, 2)), np.zeros((env.num_targets, 2)))
    env.send_messages([Message(sender=0, recipient=2, content=1, team=Team.CAMERA), Message(sender=2, recipient=0, content=1, team=Team.CAMERA)])
    env.send_messages(Message(sender=5, recipient=None, content=1, team=Team.TARGET))      # a broadcast: every target, the sender included
    env.step(idle)
    assert env.camera_comm_matrix[0, 2] == env.camera_comm_matrix[2, 0] == 4 and env.camera_comm_matrix.sum() == 8
    assert (env.target_comm_matrix[5] == 4).all() and env.target_comm_matrix.sum() == 4 * env.num_targets
    env.send_messages(Message(sender=1, recipient=3, content=1, team=Team.CAMERA))
    env.step(idle)
    assert env.camera_comm_matrix[0, 2] == 3 and env.camera_comm_matrix[1, 3] == 4
    image = env.render(mode='rgb_array', window_size=200)
    scene = R.scene_of_engine(env.engine, 0, headings=env.target_orientations)
    prims = RC.display_list(scene, (env.camera_comm_matrix, env.target_comm_matrix), 4)
    assert sum(p['kind'] == 'line' for p in prims) == 2 + 2 + 3 + 3 * (env.num_targets - 1)
    _same_outside_the_rim(image, RC.rasterise(prims, 200), RC.rim(prims, 200), 'N = 1')
    for _ in range(4):
        env.step(idle)
    assert not env.camera_comm_matrix.any() and not env.target_comm_matrix.any()
    env.send_messages(Message(sender=1, recipient=3, content=1, team=Team.CAMERA))
    env.step(idle)
    env.reset()
    assert not env.camera_comm_matrix.any()
    plain = R.display_list(R.scene_of_engine(env.engine, 0, headings=env.target_orientations))
    _same_outside_the_rim(env.render(mode='rgb_array', window_size=64), R.rasterise(plain, 64), R.rim(plain, 64), 'N = 1 behind reset')
    env.close()


def test_the_batched_class():
    import mate_amd
    env = mate_amd.BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=4, seed=2, render_communication=20)
    env.enable_greedy_policies()
    env.reset()
    for _ in range(3):
        env.engine.step_greedy(auto_reset=env.auto_reset)
    cam, tgt = env.communication_trace()
    assert cam.shape == (4, 4, 4) and tgt.shape == (4, 8, 8) and cam.dtype == torch.uint8 and cam.any()
    frames = env.render(envs=(2, 0), size=200).cpu().numpy()
    for k, e in enumerate((2, 0)):
        prims = _restated(env.engine, e)
        assert any(p['kind'] == 'line' for p in prims)
        _same_outside_the_rim(frames[k], RC.rasterise(prims, 200), RC.rim(prims, 200), ('batched', e))
    with pytest.raises(ValueError):
        mate_amd.BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=4, render_communication=0)
    env.close()


def _decode_png(path):
    with open(path, 'rb') as fh:
        data = fh.read()
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    at, body, shape = 8, b'', None
    while at < len(data):
        n, = struct.unpack('>I', data[at:at + 4])
        tag, chunk = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        if tag == b'IHDR':
            shape = struct.unpack('>II', chunk[:8])
        if tag == b'IDAT':
            body += chunk
        at += 12 + n
    rows = np.frombuffer(zlib.decompress(body), dtype=np.uint8).reshape(shape[1], 1 + shape[0] * 3)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(shape[1], shape[0], 3)


def test_the_evaluate_tool_draws_the_arrows(tmp_path):
    import mate_amd
    from mate_amd import evaluate
    common = ['--config', 'MATE-4v8-9.yaml', '--policy', 'greedy', '--max-episode-steps', '5', '--frame-size', '64']
    evaluate.main(common + ['--save-frames', str(tmp_path / 'plain')])
    evaluate.main(common + ['--save-frames', str(tmp_path / 'arrows'), '--render-communication'])
    names = sorted(os.listdir(tmp_path / 'arrows'))
    assert names == sorted(os.listdir(tmp_path / 'plain')) and len(names) == 6
    plain, arrows = (np.stack([_decode_png(tmp_path / d / n) for n in names]) for d in ('plain', 'arrows'))
    assert np.array_equal(plain[0], arrows[0]) and (plain[1:] != arrows[1:]).any()      # behind the reset nobody has talked yet; the cameras' first exchange shows from the first step on
    evaluate.main(['--config', 'MATE-4v8-9.yaml', '--policy', 'greedy', '--max-episode-steps', '20', '--num-envs', '4', '--episodes', '4', '--frame-size', '32',
                   '--save-frames', str(tmp_path / 'many'), '--render-communication', '5'])
    assert len(os.listdir(tmp_path / 'many')) >= 2
    # the tool's own loop with an environment we keep: the last PNG decodes to the pixels Engine.render gives for the state the loop ended in
    env = mate_amd.MultiAgentTracking('MATE-4v8-9.yaml', max_episode_steps=4)
    env.enable_greedy_policies()
    env.enable_render_communication(20)
    env.seed(1)
    saver = evaluate.FrameSaver(str(tmp_path / 'kept'), size=72)
    evaluate.evaluate(env, None, frames=saver)
    assert env.engine.communication_trace('camera').any()
    assert np.array_equal(_decode_png(saver.written[-1]), env.engine.render([0], size=72, headings=env.target_orientations[None])[0].cpu().numpy())
    prims = _restated(env.engine, 0, headings=env.target_orientations)
    assert any(p['kind'] == 'line' for p in prims)
    _same_outside_the_rim(_decode_png(saver.written[-1]), RC.rasterise(prims, 72), RC.rim(prims, 72), 'tool')
    env.close()
