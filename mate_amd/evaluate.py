"""Episode harness of the N=1 API: the counterpart of the reference's evaluation loop (mate/evaluate.py:85-167).

The reference wraps the environment so that one team is played by built-in agents (`mate.MultiCamera`), runs one episode
with the other team's agents and reports a status row: episode step, delivered cargoes, step reward, target-team episode
reward, steps per cargo, mean transport rate, mean coverage rate, normalised episode reward, FPS
(mate/evaluate.py:52-73, 129-143).  `evaluate()` below runs the same loop on `mate_amd.MultiAgentTracking` with the same
status keys and the same update rule (the row is kept from the first delivery on, or at `done`).  Both teams act through
`joint_policy`; by default they are the reference's GreedyCameraAgent / GreedyTargetAgent computed ON THE DEVICE
(`Engine.step_greedy`), so the whole loop is one policy launch + one step launch per step.

    python -m mate_amd.evaluate [--config MATE-4v2-9.yaml] [--seed 0] [--episodes 1] [--policy greedy|random]

With `--num-envs N` the episodes run on the batched environment instead, N at a time under the on-device agents, and the report is
the mean and standard deviation over the first `--episodes` episode records (Engine.enable_episode_records: the per-episode metrics
of the reference's example trainers) of the columns EPISODE_REPORT.

    python -m mate_amd.evaluate --num-envs 4096 --episodes 4096 [--policy greedy|random] [--team target|camera]
"""
import argparse
import time
from collections import OrderedDict

import numpy as np

__all__ = ['COLUMNS', 'EPISODE_REPORT', 'evaluate', 'evaluate_batched', 'random_policy', 'format_row', 'build_parser']

# the columns of an episode record (Engine.EPISODE_COLUMNS) the batched form reports: the three episode_ sums, the five means, the two last values
EPISODE_REPORT = slice(5, 15)

# name -> format of the reference's table (mate/evaluate.py:52-71)
COLUMNS = OrderedDict([
    ('Step', '{:d}'.format), ('Cargo', '{:d}'.format), ('Reward', '{:+.2f}'.format), ('Target Episode Reward', '{:+.2f}'.format),
    ('Step / Cargo', '{:.1f}'.format), ('Mean Transport Rate', lambda x: f'{100.0 * x:.3f}%'),
    ('Mean Coverage Rate', lambda x: f'{100.0 * x:.3f}%'), ('Normalized Target Episode Reward', '{:+.5f}'.format), ('FPS', '{:.1f}'.format),
])


def random_policy(seed=0):
    """Uniform samples of the two joint action spaces (examples/random.py)."""
    rng = np.random.RandomState(seed)

    def act(env, observations, infos):
        cam = rng.uniform(-1.0, 1.0, (env.num_cameras, 2)) * np.array([env.camera_rotation_step, env.camera_zooming_step])
        tgt = np.stack([rng.uniform(-1.0, 1.0, 2) * env.targets[t].step_size for t in range(env.num_targets)])
        return cam, tgt
    return act


def format_row(values):
    return '|'.join([''] + [f' {fmt(v)} ' for fmt, v in zip(COLUMNS.values(), values)] + [''])


class _EpisodeLog:
    """Running quantities behind one status row (mate/evaluate.py:129-139)."""

    def __init__(self, env):
        self.env = env
        self.episode_reward = 0.0
        self.coverage_sum = 0.0
        self.steps = 0
        self.started = time.perf_counter()

    def row(self, step_reward):
        env = self.env
        self.steps += 1
        self.episode_reward += step_reward
        self.coverage_sum += env.coverage_rate
        delivered = env.num_delivered_cargoes
        return OrderedDict(zip(COLUMNS, (
            env.episode_step, delivered, step_reward, self.episode_reward,
            env.episode_step / delivered if delivered > 0 else np.nan,
            env.mean_transport_rate, self.coverage_sum / self.steps,
            self.episode_reward / env.max_target_team_episode_reward,
            env.episode_step / (time.perf_counter() - self.started))))


def write_png(path, image):
    """An RGB uint8 [H, W, 3] array as a PNG file, with the standard library only: 8-bit truecolour, filter 0 on every row, one IDAT chunk."""
    import struct
    import zlib
    image = np.ascontiguousarray(image, dtype=np.uint8)
    assert image.ndim == 3 and image.shape[2] == 3, image.shape
    height, width = image.shape[:2]

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    rows = np.concatenate([np.zeros((height, 1), dtype=np.uint8), image.reshape(height, width * 3)], axis=1)
    with open(path, 'wb') as fh:
        fh.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', width, height, 8, 2, 0, 0, 0))
                 + chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) + chunk(b'IEND', b''))


class FrameSaver:
    """--save-frames: every `every`-th call writes `directory`/frame_<call>.png from the picture `draw(size)` returns (uint8 [size, size, 3])."""

    def __init__(self, directory, size=800, every=1):
        import os
        assert every >= 1
        os.makedirs(directory, exist_ok=True)
        self.directory, self.size, self.every, self.calls, self.written = directory, int(size), int(every), 0, []

    def __call__(self, draw):
        import os
        if self.calls % self.every == 0:
            self.written.append(os.path.join(self.directory, 'frame_%06d.png' % self.calls))
            write_png(self.written[-1], draw(self.size))
        self.calls += 1


def evaluate(env, joint_policy=None, verbose=False, history=None, frames=None):
    """One episode (mate/evaluate.py:85-167).  `joint_policy(env, (camera_obs, target_obs), (camera_infos, target_infos))`
    returns the joint action of both teams; None = the on-device Greedy agents of both teams
    (`env.enable_greedy_policies()` must then precede this call).  Returns the reference's status dict -- the row of
    the last step once a cargo has been delivered or the episode is done, else empty; `history` (a list) receives
    every step's row.  The loop ends at `max_episode_steps` like the reference's, one call before the environment's own
    time-limit `done`.  `frames` (a FrameSaver): the picture behind the reset and behind every step (mate/evaluate.py's env.render())."""
    observations, infos, status = env.reset(), None, {}
    draw = lambda size: env.render(mode='rgb_array', window_size=size)      # noqa: E731
    if frames is not None:
        frames(draw)
    log = _EpisodeLog(env)
    if verbose:
        print('|'.join([''] + [f' {name} ' for name in COLUMNS] + ['']))
    done = False
    while not done and env.episode_step < env.max_episode_steps:
        if joint_policy is None:
            observations, rewards, done, infos = env.step_greedy()
        else:
            observations, rewards, done, infos = env.step(joint_policy(env, observations, infos))
        row = log.row(rewards[1])                 # the target team's reward, as in the reference's single-team loop
        if row['Cargo'] > 0 or done:
            status = dict(row)
        if history is not None:
            history.append(dict(row))
        if verbose:
            print(format_row(list(row.values())))
        if frames is not None:
            frames(draw)
    return status


def evaluate_batched(env, episodes, policy='greedy', chunk=16, seed=0, frames=None):
    """Runs `env` (a BatchedMultiAgentTracking built with episode_records) under the on-device agents -- 'greedy': both teams' scripted
    agents, fused `chunk` frames per launch where both are the Greedy ones; 'random': the uniform policy -- until `episodes` episode
    records have arrived.  An environment built with single_agent = ... runs a uniformly random learner in the seat (a generator seeded with
    `seed`) among the on-device teammates, whatever `policy`.  Returns them, oldest first, [episodes, 16] f64 on the host.  `frames` (a
    FrameSaver): the picture of environment 0 behind the reset and behind every `chunk` frames (no headings: the engine keeps none)."""
    import torch
    env.reset()
    draw = lambda size: env.render((0,), size=size)[0].cpu().numpy()      # noqa: E731
    if frames is not None:
        frames(draw)
    # (an active communication channel is like a non-Greedy opponent: the fused launch delivers every message, so per-step calls)
    fused = policy == 'random' or (env.target_agent == 'greedy' and env.camera_agent == 'greedy' and not any(env.engine.mixtures) and not env.engine.channel_active())
    rows, have = [], 0
    single = getattr(env, 'single_agent', None)
    if single:
        generator = torch.Generator(device=env.device).manual_seed(int(seed))
        high = torch.tensor([env.engine._cfg.camera_rotation_step, env.engine._cfg.camera_zooming_step] if single == 'camera' else [env.engine._cfg.target_step_size] * 2,
                            dtype=torch.float64, device=env.device)
    limit = (env.max_episode_steps + chunk) * (2 + episodes // env.num_envs)      # (every environment ends an episode within max_episode_steps frames)
    for _ in range(0, limit, chunk):
        if single:
            for _ in range(chunk):
                env.step_single((torch.rand((env.num_envs, 2), generator=generator, dtype=torch.float64, device=env.device) * 2.0 - 1.0) * high)
        elif policy == 'random':
            env.rollout_random(chunk)
        elif fused:
            env.rollout_greedy(chunk)
        else:
            for _ in range(chunk):
                env.engine.step_greedy(auto_reset=env.auto_reset)
        if frames is not None:
            frames(draw)
        records = env.episodes()
        rows.append(torch.stack([records[name] for name in env.engine.EPISODE_COLUMNS], dim=1).cpu())
        have += rows[-1].shape[0]
        if have >= episodes:
            return torch.cat(rows)[:episodes].numpy()
    raise RuntimeError(f'{have} of {episodes} episode records after {limit} frames')


def parse_mixture(text):
    """'naive' or 'greedy:1,random:1' -> {name: weight} as Engine.set_opponent_mixture takes it (argparse reports a ValueError as a usage error)."""
    from .engine import SCRIPTED_AGENTS, mixture_table
    mixture = {}
    for part in text.split(','):
        name, _, weight = part.strip().partition(':')
        if name in mixture or name == 'external' or name not in SCRIPTED_AGENTS:
            raise ValueError(f'{name!r}: the candidates are {SCRIPTED_AGENTS[:4]}, each at most once')
        mixture[name] = float(weight) if weight else 1.0
    mixture_table(mixture)
    return mixture


def parse_rate(text):
    """A dropout rate in [0, 1] (argparse reports a ValueError as a usage error)."""
    from .engine import channel_settings
    return channel_settings(None, float(text))[1]


def parse_limit(text):
    """A range limit: a non-negative number (argparse reports a ValueError as a usage error)."""
    from .engine import channel_settings
    limit = float(text)
    if limit < 0.0:
        raise ValueError('a communication range is not negative')
    channel_settings(limit, 0.0)
    return limit


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m mate_amd.evaluate', description=__doc__.split('\n')[0])
    ap.add_argument('--config', '--cfg', default='MATE-4v2-9.yaml')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--episodes', type=int, default=1)
    ap.add_argument('--policy', choices=['greedy', 'random'], default='greedy')
    ap.add_argument('--camera-agent', choices=['greedy', 'heuristic'], default='greedy',
                    help="the scripted agent of the camera team under --policy greedy (mate.evaluate's --camera-agent)")
    ap.add_argument('--target-agent', choices=['greedy', 'heuristic'], default='greedy',
                    help="the scripted agent of the target team under --policy greedy (mate.evaluate's --target-agent)")
    ap.add_argument('--camera-mixture', type=parse_mixture, default=None, metavar='NAME[:W][,NAME[:W]...]',
                    help="a per-episode opponent mixture as the camera team under --policy greedy, e.g. greedy:1,random:1 "
                         "(MixtureCameraAgent over greedy, heuristic, naive, random; in place of --camera-agent)")
    ap.add_argument('--target-mixture', type=parse_mixture, default=None, metavar='NAME[:W][,NAME[:W]...]',
                    help="... as the target team, e.g. naive (MixtureTargetAgent; in place of --target-agent)")
    ap.add_argument('--no-communication', choices=['both', 'camera', 'target', 'none'], default='none',
                    help="disable intra-team communication of the scripted agents under --policy greedy (mate.evaluate's --no-communication: mate.NoCommunication)")
    ap.add_argument('--message-dropout', type=parse_rate, default=0.0, metavar='RATE',
                    help='drop every message of the scripted agents with this probability (mate.RandomMessageDropout)')
    ap.add_argument('--communication-range', type=parse_limit, default=None, metavar='LIMIT',
                    help='deliver a message only between agents at most this far apart (mate.RestrictedCommunicationRange)')
    ap.add_argument('--max-episode-steps', type=int, default=None)
    ap.add_argument('--verbose', action='store_true')
    ap.add_argument('--num-envs', type=int, default=None,
                    help='run the batched environment, this many episodes at a time, and report episode records (without: the N = 1 loop)')
    ap.add_argument('--single-agent', choices=['camera', 'target'], default=None,
                    help='with --num-envs: a uniformly random learner in ONE seat of that team among on-device Greedy teammates (mate.SingleCamera / mate.SingleTarget); '
                         'the agent and mixture flags keep their meaning for the opposing team')
    ap.add_argument('--team', choices=['camera', 'target'], default='target',
                    help='with --num-envs: the team whose rewards the records hold (num_tracked is kept for the camera team)')
    ap.add_argument('--save-frames', default=None, metavar='DIR',
                    help="write the episode's pictures as DIR/frame_<n>.png (mate.evaluate's --save-video: rgb_array frames rasterised on the device; "
                         'with --num-envs: environment 0)')
    ap.add_argument('--frame-size', type=int, default=800, metavar='S', help='with --save-frames: S x S pixels')
    ap.add_argument('--frame-every', type=int, default=1, metavar='K',
                    help='with --save-frames: every K-th picture (a picture per step; with --num-envs: per launch of 16 frames)')
    ap.add_argument('--render-communication', type=int, nargs='?', const=20, default=None, metavar='DURATION',
                    help="with --save-frames and --policy greedy: draw intra-team messages as dashed arrows for DURATION steps each, default 20 (mate.evaluate's "
                         '--render-communication: mate.RenderCommunication; the random policy sends no messages, so the flag has no effect there)')
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    import mate_amd
    frames = FrameSaver(args.save_frames, args.frame_size, args.frame_every) if args.save_frames else None
    overrides = {} if args.max_episode_steps is None else {'max_episode_steps': args.max_episode_steps}
    if args.num_envs is not None:
        from .engine import Engine
        env = mate_amd.BatchedMultiAgentTracking(args.config, num_envs=args.num_envs, seed=args.seed, episode_records=args.team,
                                                 target_agent=args.target_agent, camera_agent=args.camera_agent,
                                                 target_mixture=args.target_mixture, camera_mixture=args.camera_mixture,
                                                 no_communication=args.no_communication, message_dropout=args.message_dropout,
                                                 communication_range=args.communication_range, single_agent=args.single_agent,
                                                 render_communication=args.render_communication if frames is not None and args.policy == 'greedy' else None, **overrides)
        if args.policy == 'greedy':
            env.enable_greedy_policies()
        records = evaluate_batched(env, args.episodes, args.policy, seed=args.seed, frames=frames)
        names = Engine.EPISODE_COLUMNS[EPISODE_REPORT]
        print(f'{len(records)} episodes of {args.config}, {args.num_envs} at a time, team {args.team}:')
        for name, column in zip(names, records[:, EPISODE_REPORT].T):
            print(f'  {name}: {column.mean():.6g} +- {column.std():.6g}')
        env.close()
        return records
    env = mate_amd.MultiAgentTracking(args.config, no_communication=args.no_communication, message_dropout=args.message_dropout,
                                      communication_range=args.communication_range, **overrides)
    if args.policy == 'greedy':
        agents = {'target_agent': args.target_agent}
        if args.camera_agent != 'greedy':
            agents['camera_agent'] = args.camera_agent
        if args.target_mixture is not None:
            agents['target_mixture'] = args.target_mixture
        if args.camera_mixture is not None:
            agents['camera_mixture'] = args.camera_mixture
        env.enable_greedy_policies(**agents)
    if args.render_communication is not None and frames is not None and args.policy == 'greedy':
        env.enable_render_communication(args.render_communication)
    env.seed(args.seed)
    rows = []
    for episode in range(args.episodes):
        status = evaluate(env, None if args.policy == 'greedy' else random_policy(args.seed + episode), verbose=args.verbose, frames=frames)
        rows.append(status)
        print(f'episode {episode}: ' + ', '.join(f'{k}: {fmt(status[k])}' for k, fmt in COLUMNS.items() if k in status))
    return rows


if __name__ == '__main__':
    main()
