#!/usr/bin/env python3
"""Generator of tests/golden/render_comm_*.npz: the reference's own display list WITH RenderCommunication's arrows.

The reference's RenderCommunication wrapper and render() run unchanged over the gym stand-in, as in make_render_golden.py, with render_recorder.py as
`mate.assets.pygletrendering` plus the two classes it lacks, Line and LineStyle (added here: a two-vertex primitive that records its stipple).  Greedy agents play
both teams.  Per scene the file holds what make_render_golden.py stores (the full primitive list in order, the state to import, the knots, the view masks) and
  comm/camera, comm/target     the wrapper's two comm_matrix arrays at the recorded frame
  comm/duration                its duration
  edges/camera, edges/target   per step of the episode, the messages the wrapper saw in message_buffers ahead of that step, [steps][sender][recipient] uint8
  list/stipple                 per primitive, the line's stipple pattern (0 where it has none)
Arrays and names only: data, no program text.  A scene whose rim pixels (tests/render_comm_ref.py: rim -- band outlines and dash switches) exceed 0.1 % of a frame
at a size the tests use is refused: choose another step.

    MATE_REFERENCE=<checkout of XuehaiPan/mate> python tests/golden/make_render_comm_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_render_golden as MR  # noqa: E402  (injects render_recorder as the reference's rendering module)
import render_comm_ref as RC  # noqa: E402  (tests/render_comm_ref.py: pure NumPy, shared with the tests)
import render_recorder  # noqa: E402

MG, mate = MR.MG, MR.mate


class LineStyle:
    def __init__(self, style):
        self.style = style


class Line(render_recorder.Geom):
    def __init__(self, start=(0.0, 0.0), end=(0.0, 0.0)):
        super().__init__()
        self.start, self.end = start, end
        self.linewidth = render_recorder.LineWidth(1)
        self.add_attr(self.linewidth)

    def draw1(self, pen):
        pen.emit('line', [self.start, self.end])
        pen.out[-1]['stipple'] = next((a.style for a in self.attrs if isinstance(a, LineStyle)), 0xFFFF)


render_recorder.Line, render_recorder.LineStyle = Line, LineStyle

RIM_SHARE = 1e-3


def edges_of(env):
    """What RenderCommunication.step is about to read: one matrix per team of the messages waiting in message_buffers."""
    out = []
    for n, buffer in zip((env.num_cameras, env.num_targets), env.unwrapped.message_buffers):
        m = np.zeros((n, n), dtype=np.uint8)
        for packs in buffer.values():
            for message in packs:
                m[message.sender, message.recipient] = 1
        out.append(m)
    return out


def run(name, seed, steps, duration, wrap=None, tweak=None):
    """Greedy against Greedy under RenderCommunication for `steps` steps; returns the wrapped environment and the per-step edges."""
    env = mate.make('MultiAgentTracking-v0', config=RC.CONFIGS[name])
    if wrap:
        env = wrap(env)
    env = mate.RenderCommunication(env, duration=duration)
    env.seed(seed)
    cam_obs, tgt_obs = env.reset()
    if tweak:
        tweak(env.unwrapped)
    cams, tgts = MR.greedy_agents(env, seed)
    mate.group_reset(cams, cam_obs)
    mate.group_reset(tgts, tgt_obs)
    infos, edges = (None, None), ([], [])
    for step in range(steps):
        cam_act = np.asarray(mate.group_step(env, cams, cam_obs, infos[0]), dtype=np.float64).reshape(env.num_cameras, 2)
        tgt_act = np.asarray(mate.group_step(env, tgts, tgt_obs, infos[1]), dtype=np.float64).reshape(env.num_targets, 2)
        for team, m in enumerate(edges_of(env)):
            edges[team].append(m)
        (cam_obs, tgt_obs), _, done, infos = env.step((cam_act, tgt_act))
        assert not done, (name, seed, step)
    return env, edges


def record(name, wrapped, edges):
    env = wrapped.unwrapped
    wrapped.render(mode='rgb_array', window_size=64)
    recorded = env.viewer.recorded
    drawn = [p for p in recorded if p['kind'] != 'image']
    kinds = {'polygon': 0, 'polyline': 1, 'line': 2}
    st, dyn = MG.snapshot_static(env), MG.snapshot_dynamic(env)
    out = {'config_file': np.array(RC.CONFIGS[name]), 'num_images': np.int64(len(recorded) - len(drawn)),
           'list/kind': np.array([kinds[p['kind']] for p in drawn], dtype=np.int64),
           'list/start': np.cumsum([0] + [len(p['v']) for p in drawn]).astype(np.int64),
           'list/vertices': np.concatenate([p['v'] for p in drawn]).astype(np.float64),
           'list/rgba': np.array([p['rgba'] for p in drawn], dtype=np.float64), 'list/width': np.array([p['width'] for p in drawn], dtype=np.float64),
           'list/stipple': np.array([p.get('stipple', 0) for p in drawn], dtype=np.int64),
           'cam_radius': np.float64(env.cameras[0].radius), 'cam_area': np.float64(env.cameras[0].min_viewing_angle * env.cameras[0].max_sight_range ** 2),
           'comm/camera': np.asarray(wrapped.camera_comm_matrix, dtype=np.int64), 'comm/target': np.asarray(wrapped.target_comm_matrix, dtype=np.int64),
           'comm/duration': np.int64(wrapped.duration), 'edges/camera': np.array(edges[0], dtype=np.uint8), 'edges/target': np.array(edges[1], dtype=np.uint8)}
    state = {'cam_xy': st['cam_xy'], 'cam_phi': dyn['cam_phi'], 'cam_theta': dyn['cam_theta'], 'obs_xyr': st['obs_xyr'], 'tgt_xy': dyn['tgt_xy'],
             'tgt_capacity': st['tgt_capacity'], 'tgt_goals': dyn['tgt_goals'], 'bounties': dyn['bounties'], 'remaining_cargoes': dyn['remaining_cargoes'],
             'awaiting_cargo_counts': dyn['awaiting_cargo_counts'], 'camera_target_view_mask': dyn['camera_target_view_mask'],
             'target_camera_view_mask': dyn['target_camera_view_mask'], 'target_orientations': np.asarray(env.target_orientations, dtype=np.float64).copy()}
    out.update({'state/' + k: np.asarray(v) for k, v in state.items()})
    for k in ('camera_obstacle_view_mask',):
        out['import/' + k] = np.asarray(st[k])
    for k in ('tgt_colliding', 'tgt_empty_bits', 'tgt_goal_bits', 'freights', 'target_steps', 'tracked_steps', 'num_delivered_cargoes', 'episode_reward',
              'delayed_episode_reward', 'episode_step', 'tracked_bits', 'target_obstacle_view_mask', 'target_target_view_mask', 'camera_camera_view_mask'):
        out['import/' + k] = np.asarray(dyn[k])
    out['knots/phis'], out['knots/rhos'], out['knots/count'] = st['lut_phis'], st['lut_rhos'], st['lut_count']
    out['max_episode_steps'] = np.int64(env.max_episode_steps)
    path = os.path.join(HERE, 'render_comm_' + name + '.npz')
    np.savez_compressed(path, **out)
    prims, _, fx = RC.load_recording(path)
    for size in RC.SIZES[name]:
        share = RC.rim(prims, size).mean()
        assert share <= RIM_SHARE, f'{name} at {size}: {share:.2%} rim pixels: choose another step'
    lines = [p for p in prims if p['kind'] == 'line']
    print(path, os.path.getsize(path), 'bytes', len(prims), 'primitives', len(lines), 'lines', 'alphas', sorted({round(p['rgba'][3], 3) for p in lines}),
          'camera pairs', int((fx['comm/camera'] > 0).sum()), 'target pairs', int((fx['comm/target'] > 0).sum()))


def main():
    for name, (seed, steps, duration, wrap, tweak) in RC.RECIPES.items():
        wrapper = (lambda env: mate.NoCommunication(env, team='camera')) if wrap == 'no_camera_communication' else None
        record(name, *run(name, seed, steps, duration, wrapper, MG.tweak_few_cargoes if tweak == 'few_cargoes' else None))


if __name__ == '__main__':
    main()
