"""Host side of the episode records (csrc/episode_rows.hpp, mate_engine_enable_episode_records): the contract's restatement
(tests/episode_ref.py: EpisodeSums) against the restated callback of the reference's trainers (MetricCollector / on_episode_end) over the
fragment fixtures, in both forms; the header, the column tuple and the evaluate command's arguments (the kernel's resource record
and the source digest: tests/test_unit_resources.py).  No GPU.

Bound of the fixture comparisons: 1e-12 absolute.  The contract adds in step order, np.mean / np.sum pairwise; the sums have at most 24 f64
terms below 8 each (tests/test_gpu_fragment.py uses the same bound with the same reasoning), so their roundings differ by a few 2^-50."""
import os
import re

import numpy as np
import pytest

import episode_ref as R
import golden_util as G
from test_fragment_host import FIXTURES, fragments_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-12
CHECKED = ('raw_reward', 'normalized_raw_reward', 'coverage_rate', 'real_coverage_rate', 'mean_transport_rate', 'num_delivered_cargoes',
           'episode_raw_reward', 'episode_normalized_raw_reward')


def _team_of(fx):
    team = 0 if str(fx['learner_team']) == 'camera' else 1
    return team, int(fx['num_cameras'] if team == 0 else fx['num_targets'])


def _compare(name, records, metrics):
    assert len(records) == len(metrics) == 2, name            # each fixture holds two episodes
    for record, expect in zip(records, metrics):
        got = dict(zip(R.COLUMNS, record))
        for key in CHECKED:
            error = abs(got[key] - expect[key])
            print(f'{name} {key}: {got[key]!r} against {expect[key]!r}, error {error:.3e}')
            assert error <= BOUND, key


@pytest.mark.parametrize('name', FIXTURES)
def test_fragment_form_equals_the_callback_over_the_fixture_fragments(name):
    fx = G.load(name + '.npz')
    team, agents = _team_of(fx)
    assert [str(k) for k in fx['info_names']] == ['raw_reward', 'normalized_raw_reward', 'coverage_rate', 'real_coverage_rate', 'mean_transport_rate',
                                                  'num_delivered_cargoes']
    sums, collector = R.EpisodeSums(team, agents, int(fx['num_cameras'])), R.MetricCollector()
    records, metrics, length = [], [], 0
    for frames, dones, info in zip(fx['skip/frames'], fx['skip/dones'], fx['skip/info']):
        raw, norm = float(info[0]), float(info[1])
        rewards = [raw, 0.0, 0.0, norm] if team == 0 else [0.0, raw, norm, 0.0]
        length += int(frames)
        collector.add([dict(zip((str(k) for k in fx['info_names']), info))] * agents)
        if sums.fragment(frames, bool(dones.all()), rewards, info[2:6]):
            records.append(sums.record(0, len(records) + 1, length))
            metrics.append(collector.episode_end())
            collector, length = R.MetricCollector(), 0
    for record in records:
        assert record[3] == record[4] and record[2] < record[3]      # frames == length: whole episodes, several frames per learner step
    _compare(name, records, metrics)


@pytest.mark.parametrize('name', FIXTURES)
def test_frame_form_equals_the_callback_over_the_fixture_frames(name):
    fx = G.load(name + '.npz')
    team, agents = _team_of(fx)
    Nc, Nt = int(fx['num_cameras']), int(fx['num_targets'])
    sums, collector = R.EpisodeSums(team, agents, Nc), R.MetricCollector()
    records, metrics, length = [], [], 0
    for record, words in zip(fx['frame/scalars'], fx['frame/view_words']):
        length += 1
        popcount = R.view_popcount(words, Nc, Nt)
        info = R.frame_infos(record, team)
        if team == 0:                                          # per camera: the targets it tracks (the callback takes the mean over the cameras)
            per_camera = [sum((int(words[(c * Nt + t) >> 5]) >> ((c * Nt + t) & 31)) & 1 for t in range(Nt)) for c in range(Nc)]
            collector.add([dict(info, num_tracked=float(n)) for n in per_camera])
        else:
            collector.add([info] * agents)
        if sums.frame(record, popcount):
            records.append(sums.record(0, len(records) + 1, length))
            metrics.append(collector.episode_end())
            collector, length = R.MetricCollector(), 0
    for record, expect in zip(records, metrics):
        assert record[2] == record[3] == record[4]
        if team == 0:
            assert abs(record[14] - expect['num_tracked']) <= BOUND
        else:
            assert np.isnan(record[14])
        # the learner's reward without a shaped row: the team reward once per agent
        assert abs(record[7] - agents * expect['episode_raw_reward']) <= agents * BOUND
    _compare(name, records, metrics)


def test_idle_frames_and_empty_fragments_are_no_steps():
    sums = R.EpisodeSums(1, 4, 2)
    assert not sums.frame([0, 1.0, 2.0, 0.5, 0.5, 0, 0, 0.1]) and sums.steps == 0.0
    assert not sums.fragment(0, 0, [0, 0, 0, 0], [0, 0, 0, 0]) and sums.steps == 0.0
    assert sums.frame([-1.0, 1.0, 1.0, 0.5, 0.25, 0.125, 3.0, 0.5])
    record = dict(zip(R.COLUMNS, sums.record(7, 2, 1)))
    assert record['env'] == 7 and record['episode'] == 2 and record['steps'] == record['frames'] == record['length'] == 1
    assert record['episode_raw_reward'] == 1.0 and record['episode_reward'] == 4.0 and record['num_delivered_cargoes'] == 3.0 and record['team'] == 1


@pytest.fixture(scope='module')
def header():
    with open(os.path.join(ROOT, 'include', 'mate_engine.h')) as fh:
        return re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)


def test_header_declares_the_two_functions_and_the_column_count(header):
    assert re.search(r'#define\s+MATE_EPISODE_COLUMNS\s+16\b', header)
    assert re.search(r'#define\s+MATE_ABI_VERSION\s+1\b', header)
    assert re.search(r'int\s+mate_engine_enable_episode_records\s*\(\s*mate_engine\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*double\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*,\s*int64_t\s*\*\s*\w+\s*\)\s*;', header)
    assert re.search(r'int\s+mate_engine_clear_episode_records\s*\(\s*mate_engine\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;', header)
    from mate_amd import _native
    assert {'mate_engine_enable_episode_records', 'mate_engine_clear_episode_records'} <= set(_native.PROTOTYPES)
    assert len(_native.PROTOTYPES['mate_engine_enable_episode_records'][1]) == 5 and len(_native.PROTOTYPES['mate_engine_clear_episode_records'][1]) == 2


def test_sixteen_columns_by_name():
    from mate_amd.engine import Engine
    assert len(Engine.EPISODE_COLUMNS) == 16 == len(set(Engine.EPISODE_COLUMNS))
    assert Engine.EPISODE_COLUMNS == R.COLUMNS


def test_evaluate_parser_takes_num_envs_and_keeps_its_defaults():
    from mate_amd.evaluate import build_parser
    defaults = build_parser().parse_args([])
    assert defaults.num_envs is None and defaults.episodes == 1 and defaults.policy == 'greedy' and defaults.config == 'MATE-4v2-9.yaml'
    assert defaults.seed == 0 and defaults.camera_agent == 'greedy' and defaults.target_agent == 'greedy' and defaults.max_episode_steps is None
    args = build_parser().parse_args(['--num-envs', '64', '--episodes', '64', '--policy', 'random', '--target-agent', 'heuristic'])
    assert args.num_envs == 64 and args.episodes == 64 and args.policy == 'random' and args.target_agent == 'heuristic' and args.team == 'target'


def test_episode_records_argument_of_the_batched_environment():
    """Checked ahead of everything that needs a GPU, like the frame_skip arguments."""
    import inspect
    from mate_amd.environment import BatchedMultiAgentTracking
    signature = inspect.signature(BatchedMultiAgentTracking.__init__)
    assert signature.parameters['episode_records'].default is None
    with pytest.raises(AssertionError, match='episode_records'):
        BatchedMultiAgentTracking('MATE-4v2-9.yaml', num_envs=2, episode_records='both')
