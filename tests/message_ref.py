"""NumPy restatement of the learner's message router (csrc/message_rows.hpp: message_rows_kernel): who receives what under a channel, and the tag
rule of the edge counts.  The verdict is tests/channel_ref.py's channel_verdict, nothing of it is restated.  tests/test_message_host.py ties this to what
the reference's own send_messages / receive_messages / step recorded under its channel wrappers (tests/golden/message_*.npz); the GPU tests take their
expected bytes from it."""
import numpy as np

import channel_ref as C

S_MSG_DROP = 28           # the Philox stream of the routed messages' dropout draws
EDGE_NAMES = ('sent', 'delivered', 'step_edges', 'total_edges', 'agent_edges')


def draw_key(round, team, sender, recipient):
    return round << 12 | team << 8 | sender << 4 | recipient


def philox_uniforms(philox, seed, first_env, num_envs, ticks, round, team, n):
    """[N, n, n] uniforms as the launch draws them: word .x of philox(seed, global environment index, tick, 28, key) as a 32-bit uniform.
    `philox`: oracle.philox; `ticks`: [N]."""
    u = np.empty((num_envs, n, n), dtype=np.float64)
    for e in range(num_envs):
        for s in range(n):
            for r in range(n):
                x = philox(seed & 0xffffffff, seed >> 32, first_env + e, int(ticks[e]), S_MSG_DROP, draw_key(round, team, s, r))[0]
                u[e, s, r] = float(x) * 2.3283064365386963e-10
    return u


def route(payload, address, pairwise, keep):
    """One routing call of one team.  `payload` [N, n, M] or, pairwise, [N, n, n, M] ([sender][recipient]); `address` None (broadcast: every slot, the
    sender's own included) or [N, n, n], non-zero = sent; `keep` [N, n, n] bool, the channel's verdict per pair.  Returns (inbox [N, n recipient, n sender, M]
    with zeros where nothing was sent or arrived, sent [N, n, n] int8, delivered [N, n, n] int8)."""
    payload = np.asarray(payload)
    N, n = payload.shape[0], payload.shape[1]
    sent = np.ones((N, n, n), dtype=bool) if address is None else np.asarray(address) != 0
    delivered = sent & np.asarray(keep, dtype=bool)
    content = payload if pairwise else np.broadcast_to(payload[:, :, None, :], (N, n, n, payload.shape[-1]))
    inbox = np.where(delivered[..., None], content, np.zeros((), dtype=payload.dtype)).transpose(0, 2, 1, 3)
    return np.ascontiguousarray(inbox), sent.astype(np.int8), delivered.astype(np.int8)


def verdict(channel, u, positions, shape):
    """[N, n, n] bool: channel_ref.channel_verdict of the team's channel -- None (no channel: everything arrives) or the keywords of Engine.set_channel."""
    if channel is None:
        return np.ones(shape, dtype=bool)
    u = np.full(shape, np.nan) if u is None else u
    return C.channel_verdict(bool(channel.get('disabled', False)), channel.get('range_limit'), float(channel.get('dropout_rate', 0.0)), channel.get('mask'), u, positions)


class Counts:
    """The edge counts of one team over N environments under the tag rule: a (tick, episode) tag per environment; a launch that meets another tick folds
    step_edges into total_edges and zeroes it, one that meets another episode zeroes both; an environment that is not `live` keeps everything."""

    def __init__(self, num_envs, n):
        self.tick = np.full(num_envs, -1, dtype=np.int64)
        self.episode = np.full(num_envs, -1, dtype=np.int64)
        self.step_edges = np.zeros((num_envs, n, n), dtype=np.int32)
        self.total_edges = np.zeros((num_envs, n, n), dtype=np.int32)
        self.agent_edges = np.zeros((num_envs, n, 2), dtype=np.int32)

    def clear_tags(self):
        """seed(), a reset of the whole batch, import_state, enable_messages"""
        self.tick[:] = -1
        self.episode[:] = -1

    def update(self, tick, episode, delivered, live=None):
        N = len(self.tick)
        tick, episode = np.broadcast_to(np.asarray(tick, dtype=np.int64), (N,)), np.broadcast_to(np.asarray(episode, dtype=np.int64), (N,))
        live = np.ones(N, dtype=bool) if live is None else np.asarray(live, dtype=bool)
        new_episode = live & (self.episode != episode)
        new_tick = live & ~new_episode & (self.tick != tick)
        self.step_edges[new_episode] = 0
        self.total_edges[new_episode] = 0
        self.total_edges[new_tick] += self.step_edges[new_tick]
        self.step_edges[new_tick] = 0
        self.step_edges[live] += np.asarray(delivered, dtype=np.int32)[live]
        self.tick[live], self.episode[live] = tick[live], episode[live]
        self.agent_edges[live] = np.stack([self.step_edges.sum(axis=2), self.step_edges.sum(axis=1)], axis=-1)[live]
        return self


def encoded_payload(num_envs, n, width, pairwise, dtype, first_env=0):
    """Contents that say where they belong: 1 + k + width (recipient + n (sender + n env)) -- small integers, exact in f32 for the tests' shapes; a per-sender
    payload encodes recipient 0."""
    e, s, r, k = np.meshgrid(np.arange(num_envs) + first_env, np.arange(n), np.arange(n if pairwise else 1), np.arange(width), indexing='ij')
    values = (1 + k + width * (r + n * (s + n * e))).astype(dtype)
    assert values.max() < 2 ** 24
    return values if pairwise else values[:, :, 0, :]
