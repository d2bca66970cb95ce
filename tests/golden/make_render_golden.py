#!/usr/bin/env python3
"""Generator of tests/golden/render_*.npz: the reference's own display list of six scenes, for the off-screen render.

pyglet is not installed, so the reference's image cannot be had; its display list can.  The reference's render() (environment.py:986-1180) runs unchanged over
the gym stand-in, with render_recorder.py (next to this file) injected as `mate.assets.pygletrendering`: every primitive the reference hands its viewer is
recorded in order -- kind, world-space vertices after its transforms, RGBA, line width.  Per scene the file holds that list (the warehouse icons, which the
device does not draw, are counted and left out), the state to import, the cameras' knots, the view masks and target_orientations.  Arrays and names only:
data, no program text.  A scene whose rim pixels (tests/render_ref.py: rim) exceed 0.1 % of a frame at a size the tests use is refused.

    MATE_REFERENCE=<checkout of XuehaiPan/mate> python tests/golden/make_render_golden.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (puts the shim and the reference on sys.path, imports gym and mate)
import render_recorder  # noqa: E402
import render_ref  # noqa: E402  (tests/render_ref.py: pure NumPy, shared with the tests)

mate = MG.mate
if not hasattr(np, 'bool8'):
    np.bool8 = np.bool_
import mate.assets  # noqa: E402
sys.modules['mate.assets.pygletrendering'] = render_recorder
mate.assets.pygletrendering = render_recorder

SIZES = {'4v8-9_random': (64, 200, 800), '2v4-0': (64, 72, 200)}      # the sizes the tests draw a scene at (tests/test_gpu_render.py); the others: (64, 200)
RIM_SHARE = 1e-3


def greedy_agents(env, seed):
    cams = MG.GreedyCameraAgent(seed=seed + 1).spawn(env.num_cameras) if env.num_cameras else []
    tgts = MG.GreedyTargetAgent(seed=seed + 2).spawn(env.num_targets)
    return cams, tgts


def run(name, seed, steps, policy, overrides=None, tweak=None, until=None, actions=None):
    """The reference environment of scene `name` after `steps` steps (or at the first step from `steps` on where `until(env)` holds) under `policy`."""
    config = render_ref.CONFIGS[name]
    env = mate.make('MultiAgentTracking-v0', config=config, **(overrides or {}))
    env.seed(seed)
    cam_obs, tgt_obs = env.reset()
    if tweak:
        tweak(env)
    rng = np.random.RandomState(seed + 100)
    if policy == 'greedy':
        cams, tgts = greedy_agents(env, seed)
        mate.group_reset(cams, cam_obs)
        mate.group_reset(tgts, tgt_obs)
    infos = (None, None)
    for step in range(4 * steps + 400):
        if step >= steps and (until is None or until(env)):
            return env
        if actions is not None:
            cam_act, tgt_act = actions(env, rng, step)
        elif policy == 'greedy':
            cam_act = np.asarray(mate.group_step(env, cams, cam_obs, infos[0]), dtype=np.float64).reshape(env.num_cameras, 2)
            tgt_act = np.asarray(mate.group_step(env, tgts, tgt_obs, infos[1]), dtype=np.float64).reshape(env.num_targets, 2)
        else:
            cam_act, tgt_act = MG.random_actions(env, rng, step)
            cam_act, tgt_act = np.clip(cam_act, env.camera_action_space.low, env.camera_action_space.high) if env.num_cameras else cam_act, tgt_act
        (cam_obs, tgt_obs), _, done, infos = env.step((cam_act, tgt_act))
        assert not done, (config, seed, step)
    raise RuntimeError(f'{config} seed {seed}: the condition never held')


def record(name, env):
    env.render(mode='rgb_array', window_size=64)
    recorded = env.viewer.recorded
    drawn = [p for p in recorded if p['kind'] != 'image']
    st, dyn = MG.snapshot_static(env), MG.snapshot_dynamic(env)
    Nc = env.num_cameras
    out = {'config_file': np.array(render_ref.CONFIGS[name]), 'num_images': np.int64(len(recorded) - len(drawn)),
           'list/kind': np.array([0 if p['kind'] == 'polygon' else 1 for p in drawn], dtype=np.int64),
           'list/start': np.cumsum([0] + [len(p['v']) for p in drawn]).astype(np.int64),
           'list/vertices': np.concatenate([p['v'] for p in drawn]).astype(np.float64),
           'list/rgba': np.array([p['rgba'] for p in drawn], dtype=np.float64), 'list/width': np.array([p['width'] for p in drawn], dtype=np.float64),
           'cam_radius': np.float64(env.cameras[0].radius if Nc else 0.0),
           'cam_area': np.float64(env.cameras[0].min_viewing_angle * env.cameras[0].max_sight_range ** 2 if Nc else 0.0)}
    state = {'cam_xy': st['cam_xy'], 'cam_phi': dyn['cam_phi'], 'cam_theta': dyn['cam_theta'], 'obs_xyr': st['obs_xyr'], 'tgt_xy': dyn['tgt_xy'],
             'tgt_capacity': st['tgt_capacity'], 'tgt_goals': dyn['tgt_goals'], 'bounties': dyn['bounties'], 'remaining_cargoes': dyn['remaining_cargoes'],
             'awaiting_cargo_counts': dyn['awaiting_cargo_counts'], 'camera_target_view_mask': dyn['camera_target_view_mask'],
             'target_camera_view_mask': dyn['target_camera_view_mask'], 'target_orientations': np.asarray(env.target_orientations, dtype=np.float64).copy()}
    out.update({'state/' + k: np.asarray(v) for k, v in state.items()})
    # everything Engine.load_state_dict needs beyond that (tests/gpu_util.py: STATE_KEYS)
    for k in ('camera_obstacle_view_mask',):
        out['import/' + k] = np.asarray(st[k])
    for k in ('tgt_colliding', 'tgt_empty_bits', 'tgt_goal_bits', 'freights', 'target_steps', 'tracked_steps', 'num_delivered_cargoes', 'episode_reward',
              'delayed_episode_reward', 'episode_step', 'tracked_bits', 'target_obstacle_view_mask', 'target_target_view_mask', 'camera_camera_view_mask'):
        out['import/' + k] = np.asarray(dyn[k])
    if Nc:
        out['knots/phis'], out['knots/rhos'], out['knots/count'] = st['lut_phis'], st['lut_rhos'], st['lut_count']
    else:
        out['knots/phis'], out['knots/rhos'], out['knots/count'] = np.zeros((0, 1)), np.zeros((0, 1)), np.zeros(0, dtype=np.int64)
    out['max_episode_steps'] = np.int64(env.max_episode_steps)
    path = os.path.join(HERE, 'render_' + name + '.npz')
    np.savez_compressed(path, **out)
    prims, scene, _ = render_ref.load_recording(path)
    for size in SIZES.get(name, (64, 200)):
        share = render_ref.rim(prims, size).mean()
        assert share <= RIM_SHARE, f'{name} at {size}: {share:.2%} rim pixels: choose another seed'
    kinds = {k: sum(p['kind'] == k for p in recorded) for k in ('polygon', 'polyline', 'image')}
    print(path, os.path.getsize(path), 'bytes', kinds, 'tracked', int(dyn['tracked_bits'].sum()), 'sensed cameras',
          int(dyn['target_camera_view_mask'].any(axis=0).sum()) if Nc else 0)
    return env


def plant_zero_bounty(env):
    """Behind the few-cargo steps (make_golden.tweak_few_cargoes: some warehouse is emptied): the first loaded target loses its bounty.  State injection on the
    reference object, reference code untouched."""
    remaining = env.remaining_cargoes.sum(axis=-1)
    assert any(remaining[w] == 0 and env.awaiting_cargo_counts[w] == 0 for w in range(4)) and any(remaining[w] > 0 or env.awaiting_cargo_counts[w] > 0 for w in range(4))
    loaded = [t for t, g in enumerate(env.target_goals) if g >= 0]
    assert loaded and any(g < 0 or b > 0 for g, b in zip(env.target_goals, env.bounties))
    env.bounties[loaded[0]] = 0
    return env


def seam_actions(env, rng, step):
    """Every camera zooms out to the 180-degree clamp and turns; the targets wander."""
    cam = np.tile([env.camera_rotation_step, env.camera_zooming_step], (env.num_cameras, 1)).astype(np.float64)
    return cam, rng.uniform(-1.0, 1.0, size=(env.num_targets, 2)) * env.target_step_size


def seam_ready(env):
    c = env.cameras[0]
    left = MG.normalize_angle(c.orientation - c.viewing_angle / 2.0)
    return c.viewing_angle == 180.0 and left + 180.0 > 200.0


def main():
    record('4v8-9_random', run('4v8-9_random', 3, 40, 'random'))
    record('8v8-9_greedy', run('8v8-9_greedy', 5, 60, 'greedy', until=lambda env: env.tracked_bits.any() and env.target_camera_view_mask.any()))
    record('2v4-0', run('2v4-0', 7, 25, 'random'))
    record('fewcargo', plant_zero_bounty(run('fewcargo', 11, 30, 'greedy', tweak=MG.tweak_few_cargoes)))
    record('seam180', run('seam180', 13, 70, 'random', until=seam_ready, actions=seam_actions))
    record('navigation', run('navigation', 17, 30, 'random'))


if __name__ == '__main__':
    main()
