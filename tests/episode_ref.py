"""Restatements for the episode-record tests, as Python loops in f64 (no GPU, no engine).

1. The engine's contract (include/mate_engine.h, csrc/episode_rows.hpp): EpisodeSums holds one environment's running sums and takes learner
   steps of either form -- `frame` (one scalar record) or `fragment` (a fragment as the fragment launch reduced it) -- with the kernel's
   operations in the kernel's order, so that `record()` reproduces a device record bit for bit.
2. The reference's example callback (examples/utils/callbacks.py): MetricCollector.add takes the mean over the agents of each key of a step's
   infos, CustomMetricCallback.on_episode_end reduces each key over the steps (np.mean, or the last value) and adds `episode_<key>`, np.sum
   over the steps, for the keys that end in `reward`.  Only that arithmetic is restated.
"""
import numpy as np

COLUMNS = ('env', 'episode', 'steps', 'frames', 'length', 'episode_raw_reward', 'episode_normalized_raw_reward', 'episode_reward',
           'raw_reward', 'normalized_raw_reward', 'coverage_rate', 'real_coverage_rate', 'mean_transport_rate', 'num_delivered_cargoes',
           'num_tracked', 'team')
NAN = float('nan')


def view_popcount(words, num_cameras, num_targets, bit_camera_target=0):
    """Set bits among the camera -> target view bits of one environment's packed mask words."""
    bits = 0
    for k in range(num_cameras * num_targets):
        b = bit_camera_target + k
        bits += (int(words[b >> 5]) >> (b & 31)) & 1
    return bits


def agent_order_sum(row):
    total = 0.0
    for value in row:
        total = total + float(value)
    return total


class EpisodeSums:
    """One environment's running sums for `team` (0 camera, 1 target) with `agents` agents on its team and `num_cameras` cameras."""

    def __init__(self, team, agents, num_cameras):
        self.team, self.agents, self.num_cameras = int(team), int(agents), int(num_cameras)
        self.clear()

    def clear(self):
        self.steps = self.frames = 0.0
        self.raw = self.norm = self.reward = self.coverage = self.real = self.tracked = 0.0
        self.last_mtr = self.last_cargo = 0.0

    def _tracked(self, popcount):
        """popcount / Nc for the camera team where the call brought masks (popcount not None), NaN otherwise."""
        if self.team != 0 or popcount is None:
            return NAN
        return float(popcount) / float(self.num_cameras)

    def frame(self, record, popcount=None, row=None, row_nan=False):
        """One frame: `record` its scalar record [8], `popcount` of its view bits or None (no masks), `row` the learner's
        reward row of the frame or None (the team reward once per agent), `row_nan`: rows exist but not for every step.  Returns
        whether the step ended the episode; a record that says done = 2 is no step."""
        record = [float(v) for v in record]
        if record[2] == 2.0:
            return False
        camera = self.team == 0
        r = record[0] if camera else record[1]
        nr = -record[7] if camera else record[7]
        self.steps = self.steps + 1.0
        self.frames = self.frames + 1.0
        self.raw = self.raw + r
        self.norm = self.norm + nr
        self.reward = self.reward + (NAN if row_nan else agent_order_sum(row) if row is not None else agent_order_sum([r] * self.agents))
        self.coverage = self.coverage + record[3]
        self.real = self.real + record[4]
        self.last_mtr, self.last_cargo = record[5], record[6]
        self.tracked = self.tracked + self._tracked(popcount)
        return record[2] == 1.0

    def fragment(self, frames, done, rewards, info, shaped=None, popcounts=None):
        """One fragment as the fragment launch reduced it: `frames` live frames, `done`, `rewards` [4] (camera, target, normalised target,
        normalised camera), `info` [4] (the two mean coverage rates, the last mean_transport_rate and num_delivered_cargoes), `shaped`
        [agents] or None, `popcounts`: the view-bit popcounts of its live frames in frame order, or None (no masks).  frames = 0 is no step."""
        frames = int(frames)
        if frames == 0:
            return False
        camera = self.team == 0
        r = float(rewards[0] if camera else rewards[1])
        nr = float(rewards[3] if camera else rewards[2])
        self.steps = self.steps + 1.0
        self.frames = self.frames + float(frames)
        self.raw = self.raw + r
        self.norm = self.norm + nr
        self.reward = self.reward + (agent_order_sum(shaped) if shaped is not None else agent_order_sum([r] * self.agents))
        self.coverage = self.coverage + float(info[0])
        self.real = self.real + float(info[1])
        self.last_mtr, self.last_cargo = float(info[2]), float(info[3])
        if popcounts is None or not camera:
            mean = NAN
        else:
            assert len(popcounts) == frames
            total = 0.0
            for popcount in popcounts:
                total = total + self._tracked(popcount)
            mean = total / float(frames)
        self.tracked = self.tracked + mean
        return int(done) == 1

    def record(self, env, episode, length):
        """The sixteen columns at an episode's end; the sums start afresh."""
        s = self.steps
        out = np.array([float(env), float(episode), s, self.frames, float(length), self.raw, self.norm, self.reward,
                        self.raw / s, self.norm / s, self.coverage / s, self.real / s, self.last_mtr, self.last_cargo,
                        self.tracked / s, float(self.team)], dtype=np.float64)
        self.clear()
        return out


def sort_records(records):
    """[M, 16] sorted by (env, episode)."""
    records = np.asarray(records, dtype=np.float64).reshape(-1, len(COLUMNS))
    return records[np.lexsort((records[:, 1], records[:, 0]))]


def same_bits(a, b):
    """Bit for bit, NaN patterns included."""
    a, b = (np.ascontiguousarray(np.where(np.isnan(x), np.nan, x), dtype=np.float64) for x in (np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)))
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


# ---- the reference's callback
CALLBACK_REDUCTIONS = {'raw_reward': 'mean', 'normalized_raw_reward': 'mean', 'coverage_rate': 'mean', 'real_coverage_rate': 'mean',
                       'mean_transport_rate': 'last', 'num_delivered_cargoes': 'last', 'num_tracked': 'mean'}


class MetricCollector:
    def __init__(self, reductions=None):
        self.reductions = dict(CALLBACK_REDUCTIONS if reductions is None else reductions)
        self.data = {}

    def add(self, infos):
        """`infos`: one mapping per agent of the learner step."""
        for key in self.reductions:
            values = [info[key] for info in infos if key in info]
            if values:
                self.data.setdefault(key, []).append(np.mean(values))

    def collect(self):
        results = {}
        for key, series in self.data.items():
            results[key] = float(np.mean(series)) if self.reductions[key] == 'mean' else float(series[-1])
        return results

    def episode_end(self):
        """collect() and the `episode_<key>` sums of the keys that end in `reward`."""
        metrics = self.collect()
        for key in tuple(metrics):
            if key.endswith('reward') and not key.startswith(('episode', 'reward_coefficient')):
                metrics['episode_' + key] = float(np.sum(self.data[key]))
        return metrics


def frame_infos(record, team):
    """The info keys of one frame's scalar record, for `team`'s agents."""
    camera = int(team) == 0
    return {'raw_reward': float(record[0] if camera else record[1]), 'normalized_raw_reward': float(-record[7] if camera else record[7]),
            'coverage_rate': float(record[3]), 'real_coverage_rate': float(record[4]), 'mean_transport_rate': float(record[5]),
            'num_delivered_cargoes': float(record[6])}
