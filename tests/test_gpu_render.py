"""The off-screen render on the device (csrc/render_rows.hpp) against tests/render_ref.py: the reference's own recorded display lists
(tests/golden/render_*.npz) rasterised in NumPy, pixel for pixel outside the rim; the restated list on the engine's own episodes (restarts, idle
environments); indices, headings, observation types, shards, refusals, inertness, the two environment classes, the evaluate tool."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import render_ref as R
from test_render_host import GOLDEN, SIZES

pytestmark = pytest.mark.gpu
MATE_EINVAL, MATE_ESTATE = -1, -4
CUT = 6                # max_episode_steps of the episode-boundary tests: seven-frame episodes
IMPORT_KEYS = ('tgt_colliding', 'tgt_empty_bits', 'tgt_goal_bits', 'freights', 'target_steps', 'tracked_steps', 'num_delivered_cargoes', 'episode_reward',
               'delayed_episode_reward', 'episode_step', 'camera_obstacle_view_mask')


@functools.lru_cache(maxsize=None)
def _recording(name):
    return R.load_recording(os.path.join(GOLDEN, 'render_%s.npz' % name))


@functools.lru_cache(maxsize=None)
def _expected(name, size, headings=True):
    """(image, rim) of a recording at a size: computed once, shared, never written to.  headings = False: the list restated with zero headings."""
    prims, scene, _ = _recording(name)
    if not headings:
        prims = R.display_list(dict(scene, target_orientations=np.zeros(len(scene['tgt_xy']))))
    image, rim = R.rasterise(prims, size), R.rim(prims, size)
    image.setflags(write=False)
    rim.setflags(write=False)
    return image, rim


@functools.lru_cache(maxsize=None)
def _planted(name, num_envs=1, obs_dtype=torch.float32):
    """An engine whose every environment holds the recording's state, knots and -- through observe() -- view masks."""
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
    for key in ('camera_target_view_mask', 'target_camera_view_mask'):      # the planted state shows the recorded view
        assert np.array_equal(masks[key][0], scene[key].astype(bool).reshape(masks[key][0].shape)), (name, key)
    return eng


_scene_of = R.scene_of_engine


def _same_outside_the_rim(image, expected, rim, where):
    assert image.shape == expected.shape and image.dtype == np.uint8, where
    assert rim.mean() <= 1e-3, (where, rim.mean())
    differ = (image != expected).any(axis=-1) & ~rim
    assert not differ.any(), (where, int(differ.sum()), np.argwhere(differ)[:5].tolist())


def _against_the_restatement(eng, envs, size, where, masks=None):
    frames = eng.render(envs, size=size).cpu().numpy()
    for k, env in enumerate(envs):
        prims = R.display_list(_scene_of(eng, env, masks=masks))
        _same_outside_the_rim(frames[k], R.rasterise(prims, size), R.rim(prims, size), (where, env))
    return frames


# ------------------------------------------------------------------ 1. the recorded lists
@pytest.mark.parametrize('name,size', [(name, size) for name in R.SCENES for size in SIZES[name]])
def test_the_device_image_is_the_recorded_list_rasterised(name, size):
    """Every scene at 64 and 200, one at 800, one at the tile-edge size 72 (no multiple of the 16-pixel tile: the element path, partial tiles), behind a guard."""
    eng = _planted(name)
    _, scene, _ = _recording(name)
    expected, rim = _expected(name, size)
    guard = torch.full((size * size * 3 + 64,), 0x5a, dtype=torch.uint8, device=eng.device)
    out = guard[:size * size * 3].view(1, size, size, 3)
    got = eng.render([0], size=size, headings=scene['target_orientations'][None], out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and bool((guard[size * size * 3:] == 0x5a).all())
    _same_outside_the_rim(out[0].cpu().numpy(), expected, rim, (name, size))


def test_headings_null_is_zeros():
    name, size = 'fewcargo', 64
    eng = _planted(name)
    _, scene, _ = _recording(name)
    none = eng.render([0], size=size)
    zeros = eng.render([0], size=size, headings=np.zeros((1, eng.num_targets)))
    given = eng.render([0], size=size, headings=scene['target_orientations'][None])
    assert torch.equal(none, zeros) and not torch.equal(none, given)
    _same_outside_the_rim(none[0].cpu().numpy(), *_expected(name, size, headings=False), where=name)


# ------------------------------------------------------------------ 2. the engine's own episodes
def _own(n, seed, config='MATE-4v2-9.yaml', cut=None, obs_dtype=torch.float32, first_env_index=0, policies=True):
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    eng = Engine(read_config(config, **({'max_episode_steps': cut} if cut else {})), n, seed=seed, obs_dtype=obs_dtype, first_env_index=first_env_index)
    if policies:
        eng.enable_policies()
    else:
        eng.keep_masks()      # (the mask words alone: no on-device agents)
    eng.reset()
    return eng


@pytest.mark.parametrize('policies', [True, False])
def test_several_frames_repeated_and_unordered_indices(policies):
    eng = _own(5, 31, policies=policies)
    for _ in range(3):
        eng.step_random(auto_reset=1, want_masks=True)
    order = [3, 0, 3, 1, 4]
    frames = _against_the_restatement(eng, order, 64, 'k > 1')
    assert np.array_equal(frames[0], frames[2]) and not np.array_equal(frames[0], frames[1])
    for k, env in enumerate(order):
        assert torch.equal(eng.render([env], size=64)[0].cpu(), torch.from_numpy(frames[k])), env
    blind = _own(5, 31, policies=policies)      # the same steps without their masks output: the engine's own words follow them all the same
    for _ in range(3):
        blind.step_random(auto_reset=1, want_masks=False)
    assert torch.equal(blind.render(order, size=64).cpu(), torch.from_numpy(frames))
    every = eng.render(size=64)      # None: the whole batch in order
    assert every.shape == (5, 64, 64, 3) and all(torch.equal(every[env].cpu(), torch.from_numpy(frames[k])) for k, env in enumerate(order))


def test_an_environment_after_an_immediate_restart():
    eng = _own(6, 23, cut=CUT)
    restarted = None
    for s in range(CUT + 2):
        before = eng.state_dict()['episode'].copy()
        eng.step_random(auto_reset=1, want_masks=True)
        torch.cuda.synchronize()
        restarted = np.flatnonzero(eng.state_dict()['episode'] != before)
        if len(restarted):
            break
    assert restarted is not None and len(restarted) > 0
    _against_the_restatement(eng, [int(restarted[0])], 64, 'restarted')


def test_an_environment_idling_under_a_batched_restart():
    eng = _own(8, 29, cut=CUT)
    idle = None
    for s in range(3 * CUT):
        eng.step_random(auto_reset=4, want_masks=True)
        torch.cuda.synchronize()
        idle = torch.nonzero(eng.scalars[:, 2] == 2).flatten().tolist()
        if idle:
            break
    assert idle
    live = [e for e in range(8) if e not in idle][:1]
    _against_the_restatement(eng, idle[:1] + live, 64, 'idle')


def test_observation_types_and_shards_give_the_same_bytes():
    def run(**kwargs):
        eng = _own(kwargs.pop('n', 4), 37, config='MATE-4v8-9.yaml', **kwargs)
        for _ in range(4):
            eng.step_random(auto_reset=1, want_masks=True)
        return eng
    whole = run().render(size=72)
    assert torch.equal(whole, run(obs_dtype=torch.float64).render(size=72))
    assert torch.equal(whole[2:], run(n=2, first_env_index=2).render(size=72))
    assert not torch.equal(whole[0], whole[1])


def test_engine_groups_forward():
    from mate_amd.config import read_config
    from mate_amd.engine import EngineGroups
    groups = EngineGroups(read_config('MATE-4v2-9.yaml'), 4, groups=2, seed=41, policies=True)
    groups.reset()
    single = _own(4, 41)
    frames = groups.render([3, 0], size=64)
    assert torch.equal(frames, single.render([3, 0], size=64))
    groups.close()


# ------------------------------------------------------------------ 3. refusals, inertness
def test_every_refusal_changes_and_launches_nothing():
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    fresh = Engine(read_config('MATE-4v2-9.yaml'), 3, seed=1)
    size, out = 32, torch.full((3 * 32 * 32 * 3 + 16,), 0x5a, dtype=torch.uint8, device='cuda')
    call = lambda e, index, count, s, headings, ptr: e.lib.mate_engine_render(      # noqa: E731
        e._h, index, count, s, headings, ctypes.c_void_p(ptr) if ptr else None, e._stream())
    assert call(fresh, None, 1, size, None, out.data_ptr()) == MATE_ESTATE and 'before reset' in fresh.lib.mate_engine_last_error().decode()
    assert call(fresh, None, 1, 15, None, out.data_ptr()) == MATE_EINVAL      # what is wrong with the arguments comes first
    fresh.reset()
    assert call(fresh, None, 1, size, None, out.data_ptr()) == MATE_ESTATE and 'mask words' in fresh.lib.mate_engine_last_error().decode()
    from mate_amd._native import EngineError
    with pytest.raises(EngineError, match='mask words'):
        fresh.render([0], size=size)
    fresh.keep_masks()      # behind the reset: allowed, and the words read zero until a launch writes a view
    fresh.keep_masks()
    assert call(fresh, None, 1, size, None, out.data_ptr() + 8) == MATE_EINVAL
    out.fill_(0x5a)
    eng = _own(3, 1)
    before = eng.export_state().clone()
    assert call(eng, None, 0, size, None, out.data_ptr()) == MATE_EINVAL
    assert call(eng, None, 4, size, None, out.data_ptr()) == MATE_EINVAL and 'outside [0, 3)' in eng.lib.mate_engine_last_error().decode()
    assert call(eng, None, 1, 15, None, out.data_ptr()) == MATE_EINVAL and call(eng, None, 1, 4097, None, out.data_ptr()) == MATE_EINVAL
    assert call(eng, None, 1, size, None, 0) == MATE_EINVAL and call(eng, None, 1, size, None, out.data_ptr() + 8) == MATE_EINVAL
    assert '16-byte aligned' in eng.lib.mate_engine_last_error().decode()
    index = torch.tensor([0, 0, 1], dtype=torch.int32, device='cuda')
    assert call(eng, ctypes.c_void_p(index.data_ptr() + 2), 1, size, None, out.data_ptr()) == MATE_EINVAL
    for bad in ([3], [-1], [], [0, 7]):
        with pytest.raises(ValueError):
            eng.render(bad, size=size)
    with pytest.raises(ValueError):
        eng.render([0], size=8)
    with pytest.raises(ValueError):
        eng.render([0], size=size, headings=np.zeros((2, eng.num_targets)))
    torch.cuda.synchronize()
    assert bool((out == 0x5a).all()) and torch.equal(eng.export_state(), before)
    # an index on the device that the host never saw: the kernel leaves that frame alone and draws the others
    index = torch.tensor([1, 9, -2], dtype=torch.int32, device='cuda')
    assert call(eng, ctypes.c_void_p(index.data_ptr()), 3, size, None, out.data_ptr()) == 0
    torch.cuda.synchronize()
    frames = out[:3 * size * size * 3].view(3, size, size, 3)
    assert torch.equal(frames[0], eng.render([1], size=size)[0]) and bool((frames[1:] == 0x5a).all()) and bool((out[3 * size * size * 3:] == 0x5a).all())


def test_rendering_between_the_steps_changes_none_of_their_bytes():
    def run(render):
        eng = _own(8, 43, config='MATE-4v8-9.yaml', cut=12)
        seen = []
        gen = torch.Generator(device='cpu').manual_seed(5)
        for s in range(5):
            eng.step_random(auto_reset=1, want_masks=True)
            if render:
                eng.render([s % 8, 0], size=48)
            eng.step_greedy(auto_reset=3)
            if render:
                eng.render(size=32)
            act = (torch.rand((8, eng.num_cameras, 2), generator=gen, dtype=torch.float64) * 2 - 1).to(eng.device)
            eng.step_versus_greedy('camera', act, auto_reset=3)
            eng.rollout_greedy(4, auto_reset=True)
            if render:
                eng.render([7], size=16)
            torch.cuda.synchronize()
            seen.append([t.clone() for t in (eng.camera_obs, eng.target_obs, eng.scalars, eng.masks, eng.export_state())])
        return seen
    for s, (a, b) in enumerate(zip(run(False), run(True))):
        for x, y in zip(a, b):
            assert torch.equal(x, y), s


def test_the_first_render_of_a_default_engine_writes_nothing_the_caller_sees():
    """No on-device agents, as both classes build their engines by default: the first render() included, the caller-visible rows, scalars and masks and the
    records are byte for byte those of a twin that never renders."""
    def run(render):
        eng = _own(6, 47, config='MATE-4v8-9.yaml', cut=12, policies=False)
        seen = []
        for s in range(4):
            eng.step_random(auto_reset=1, want_masks=bool(s & 1))
            torch.cuda.synchronize()
            held = [t.clone() for t in (eng.camera_obs, eng.target_obs, eng.scalars, eng.masks)]
            if render:
                eng.render([s % 6, 0], size=48)
                torch.cuda.synchronize()
                for x, y in zip(held, (eng.camera_obs, eng.target_obs, eng.scalars, eng.masks)):
                    assert torch.equal(x, y), s
            seen.append(held + [eng.export_state()])
        return seen
    for s, (a, b) in enumerate(zip(run(False), run(True))):
        for x, y in zip(a, b):
            assert torch.equal(x, y), s


def test_the_batched_class_hands_out_views_a_render_leaves_alone():
    import mate_amd
    def run(render):
        env = mate_amd.BatchedMultiAgentTracking('MATE-4v2-9.yaml', num_envs=4, seed=5)
        env.reset()
        out = []
        gen = torch.Generator(device='cpu').manual_seed(9)
        for s in range(3):
            cam = (torch.rand((4, env.engine.num_cameras, 2), generator=gen, dtype=torch.float64) * 2 - 1).to(env.engine.device)
            tgt = (torch.rand((4, env.engine.num_targets, 2), generator=gen, dtype=torch.float64) * 2 - 1).to(env.engine.device)
            (cam_obs, tgt_obs), (r_cam, r_tgt), done, info = env.step((cam, tgt))
            if render:
                env.render(envs=(s, 0), size=32)      # (s = 0: the engine's first render)
            torch.cuda.synchronize()
            out.append([t.clone() for t in (cam_obs, tgt_obs, r_cam, r_tgt, done, env.engine.scalars, env.engine.masks)])
        env.close()
        return out
    for s, (a, b) in enumerate(zip(run(False), run(True))):
        for x, y in zip(a, b):
            assert torch.equal(x, y), s


# ------------------------------------------------------------------ 4. the environment classes, the tool
def test_the_single_environment_class():
    import mate_amd
    from mate_amd.utils import arctan2_deg
    env = mate_amd.MultiAgentTracking('MATE-4v8-9.yaml')
    assert 'rgb_array' in env.metadata['render.modes']
    env.seed(3)
    env.reset()
    goals, xy = env.target_goals, env._target_locations()
    for t in range(env.num_targets):      # environment.py:814-821: towards the goal
        if goals[t] >= 0:
            away = mate_amd.constants.WAREHOUSES[goals[t]] - xy[t]
            assert env.target_orientations[t] == arctan2_deg(away[1], away[0])
    rng = np.random.RandomState(0)
    for _ in range(3):
        before = env._target_locations()
        env.step((np.zeros((env.num_cameras, 2)), rng.uniform(-1, 1, size=(env.num_targets, 2)) * env.config['target']['step_size']))
        moved = env._target_locations() - before
        for t in np.flatnonzero((moved != 0).any(axis=-1)):      # environment.py:1347-1352
            assert env.target_orientations[t] == arctan2_deg(moved[t, 1], moved[t, 0])
    image = env.render(mode='rgb_array', window_size=64)
    assert isinstance(image, np.ndarray) and image.shape == (64, 64, 3) and image.dtype == np.uint8
    prims = R.display_list(_scene_of(env.engine, 0, headings=env.target_orientations))
    _same_outside_the_rim(image, R.rasterise(prims, 64), R.rim(prims, 64), 'N = 1')
    assert np.array_equal(env.render(mode='rgb_array', window_size=64), image)
    with pytest.raises(NotImplementedError):
        env.render()
    with pytest.raises(NotImplementedError):
        env.render(mode='human')
    env.close()


def test_the_batched_class():
    import mate_amd
    env = mate_amd.BatchedMultiAgentTracking('MATE-4v2-9.yaml', num_envs=4, seed=2)
    env.reset()
    env.rollout_random(3)
    frames = env.render(envs=(2, 0), size=64)
    assert frames.shape == (2, 64, 64, 3) and frames.dtype == torch.uint8 and frames.device == env.engine.device
    assert torch.equal(frames, env.engine.render([2, 0], size=64)) and env.render().shape == (1, 800, 800, 3)
    turned = env.render(envs=(2, 0), size=256, headings=np.full((2, env.engine.num_targets), 90.0))      # (at 64 pixels a target is a pixel or two)
    assert not torch.equal(turned, env.render(envs=(2, 0), size=256))
    env.close()


def test_the_evaluate_tool_saves_frames(tmp_path):
    from mate_amd import evaluate
    evaluate.main(['--config', 'MATE-2v4-0.yaml', '--policy', 'random', '--max-episode-steps', '4', '--save-frames', str(tmp_path / 'one'), '--frame-size', '48',
                   '--frame-every', '2'])
    names = sorted(os.listdir(tmp_path / 'one'))
    assert names == ['frame_000000.png', 'frame_000002.png', 'frame_000004.png']
    with open(tmp_path / 'one' / names[0], 'rb') as fh:
        assert fh.read(8) == b'\x89PNG\r\n\x1a\n'
    evaluate.main(['--config', 'MATE-2v4-0.yaml', '--policy', 'random', '--max-episode-steps', '20', '--num-envs', '4', '--episodes', '4',
                   '--save-frames', str(tmp_path / 'many'), '--frame-size', '32'])
    assert len(os.listdir(tmp_path / 'many')) >= 2
