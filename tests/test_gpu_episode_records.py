"""Per-episode metric records on the device (Engine.enable_episode_records; csrc/episode_rows.hpp, episode_kernels.hip): every stepping flow
against tests/episode_ref.py fed with the engine's OWN per-step outputs of the same run -- same operations, same order, so
the records are compared BIT FOR BIT after sorting by (env, episode) --, the append (full and partial ballots, the ring's wrap), shaped
rows and masks, graph replay, the episodes in progress across resets / seed / import_state, the refusals, the environment class and the
evaluate command.

Episode lengths: the engine ends an episode on the step AFTER max_episode_steps (the reference's time limit), so a cut of 7 gives
eight-frame episodes; `length` is the engine's own step count at the end."""
import ctypes

import numpy as np
import pytest
import torch

import episode_ref as R
import golden_util as G
from test_fragment_host import FIXTURES, fragments_of

pytestmark = pytest.mark.gpu
N_TILES = 33          # two full 16-environment tiles and a partial one
CUT = 7               # max_episode_steps: eight-frame episodes


def _engine(config, N, seed=3, cut=CUT, policies=False, obs_dtype=torch.float32):
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    eng = Engine(read_config(config, max_episode_steps=cut), N, seed=seed, obs_dtype=obs_dtype)
    if policies:
        eng.enable_policies()
    eng.reset()
    return eng


class PopCount:
    """A frame's view-bit popcount that did not come from mask words (Mirror.frames: `terms`)."""

    def __init__(self, value):
        self.value = value


class Mirror:
    """tests/episode_ref.py's sums, one per environment, fed with what the engine itself returned."""

    def __init__(self, eng, team):
        self.eng, self.team = eng, {'camera': 0, 'target': 1}[team]
        agents = eng.num_cameras if self.team == 0 else eng.num_targets
        self.sums = [R.EpisodeSums(self.team, agents, eng.num_cameras) for _ in range(eng.num_envs)]
        self.records, self.episode, self.step = [], None, None

    def before(self):
        """The episode numbers and step counts ahead of a call (a restart inside the call replaces them)."""
        state = self.eng.state_dict()
        self.episode, self.step = state['episode'].astype(np.int64).reshape(-1), state['episode_step'].astype(np.int64).reshape(-1)

    def discard(self, mask):
        for n in np.flatnonzero(np.asarray(mask)):
            self.sums[n].clear()

    def _popcount(self, words):
        if isinstance(words, PopCount):
            return words.value
        eng = self.eng
        return R.view_popcount(words, eng.num_cameras, eng.num_targets, eng.layout.bit_camera_target)

    def frames(self, scalars, masks=None, rows=None, row_nan=False, terms=None):
        """A call's frames: scalars [K, N, 8] (or [N, 8]), its masks or None, the learner's reward rows [N, A] of a one-frame call or None.
        `terms`: the camera team's reward terms [N, Nc, 7] of a one-frame call.  A per-step call with auto_reset = 1 restarts a finished
        environment INSIDE the call, and the restart writes the new episode's first view into the caller's masks: what is left of the
        terminal step's view is the num_tracked term of the reward launch (ahead of the restart, like the episode launch), so with
        `terms` the popcount is the sum of that term over the cameras -- the masks' own popcount wherever no restart replaced them."""
        s = scalars.detach().cpu().numpy().reshape(-1, self.eng.num_envs, 8)
        m = None if masks is None or self.team != 0 else masks.detach().cpu().numpy().view(np.uint32).reshape(s.shape[0], self.eng.num_envs, -1)
        if terms is not None:
            assert s.shape[0] == 1 and m is not None
            sees = terms.detach().cpu().numpy()[:, :, 5].sum(axis=1)
            restarted = s[0, :, 2] == 1.0
            assert all(self._popcount(m[0][n]) == sees[n] for n in np.flatnonzero(~restarted))
            m = [[PopCount(int(sees[n])) for n in range(self.eng.num_envs)]]
        rows = None if rows is None else rows.detach().cpu().numpy()
        for n in range(self.eng.num_envs):
            live = 0
            for f in range(s.shape[0]):
                if s[f, n, 2] == 2.0:
                    continue
                live += 1
                if self.sums[n].frame(s[f, n], None if m is None else self._popcount(m[f][n]), None if rows is None else rows[n], row_nan):
                    self.records.append(self.sums[n].record(n, self.episode[n], self.step[n] + live))
                    break

def _read(eng):
    records, dropped = eng.episode_records()
    return records.cpu().numpy(), dropped


def _assert_same(got, expect, what=''):
    got, expect = R.sort_records(got), R.sort_records(expect)
    assert got.shape == expect.shape, (what, got.shape, expect.shape)
    if not R.same_bits(got, expect):
        bad = np.argwhere(~((got == expect) | (np.isnan(got) & np.isnan(expect))))
        raise AssertionError(f'{what}: records differ at (row, column) {bad[:8].tolist()}: got {got[bad[0][0]]}, expected {expect[bad[0][0]]}')


def _random_actions(eng, gen):
    cam = ((torch.rand((eng.num_envs, eng.num_cameras, 2), generator=gen, dtype=torch.float64) * 2 - 1) * 5.0).to(eng.device)
    tgt = ((torch.rand((eng.num_envs, eng.num_targets, 2), generator=gen, dtype=torch.float64) * 2 - 1) * 20.0).to(eng.device)
    return cam, tgt


# ------------------------------------------------------------------ 1. frame form, every flow
FLOWS = {            # flow -> (the records' team, needs the on-device agents, frames per call)
    'step': ('camera', False, 1), 'versus_camera': ('camera', True, 1), 'versus_target': ('target', True, 1),
    'rollout_random': ('target', False, 5), 'rollout_greedy': ('camera', True, 5), 'rollout_versus': ('target', True, 5),
}


def _call(eng, flow, mode, gen):
    """One call of `flow`; returns (scalars, masks) of its frames."""
    cam, tgt = _random_actions(eng, gen)
    if flow == 'step':
        eng.step(cam, tgt, auto_reset=mode)
    elif flow == 'versus_camera':
        eng.step_versus_greedy('camera', cam, auto_reset=mode)
    elif flow == 'versus_target':
        eng.step_versus_greedy('target', tgt, auto_reset=mode)
    else:
        K = FLOWS[flow][2]
        if flow == 'rollout_random':
            out = eng.rollout_random(K, auto_reset=mode, want_masks=True)
        elif flow == 'rollout_greedy':
            out = eng.rollout_greedy(K, auto_reset=mode, want_masks=True)
        else:
            out = eng.rollout_versus_greedy('target', tgt, K, auto_reset=mode, want_masks=True)
        return out[2], eng._rollout['masks'][:K]
    return eng.scalars, eng.masks


@pytest.mark.parametrize('mode', [1, 0, 3])
@pytest.mark.parametrize('flow', list(FLOWS))
@pytest.mark.parametrize('config', ['MATE-4v8-9.yaml', 'MATE-2v4-0.yaml'])
def test_frame_form_in_every_flow(config, flow, mode):
    team, policies, K = FLOWS[flow]
    eng = _engine(config, N_TILES, policies=policies)
    # (a per-step call that restarts inside the call leaves the terminal view in the reward terms only: Mirror.frames)
    through_terms = K == 1 and mode == 1 and team == 'camera'
    if through_terms:
        eng.enable_reward_rows(camera=({'num_tracked': 1.0, 'raw_reward': 0.5}, 'none'), terms=True)
    eng.enable_episode_records(team)
    mirror = Mirror(eng, team)
    gen = torch.Generator(device='cpu').manual_seed(11)
    assert (CUT + 1) % K != 0 or K == 1                       # (a rollout's episodes end on an inner frame of a launch)
    ended, seen_idle = np.zeros(N_TILES, dtype=np.int64), False
    for call in range(60):
        mirror.before()
        scalars, masks = _call(eng, flow, mode, gen)
        torch.cuda.synchronize()
        if through_terms:
            mirror.frames(scalars, masks, rows=eng.camera_reward_rows, terms=eng.camera_reward_terms)
        else:
            mirror.frames(scalars, masks)
        done = (scalars.reshape(-1, N_TILES, 8)[:, :, 2] == 1).any(dim=0)
        ended += done.cpu().numpy()
        seen_idle |= bool((scalars.reshape(-1, N_TILES, 8)[:, :, 2] == 2).any())
        if mode == 0 and bool(done.any()):                    # the caller resets what has finished
            eng.reset(done)
        if ended.min() >= 3:
            break
    assert ended.min() >= 3, ended
    got, dropped = _read(eng)
    assert dropped == 0 and len(got) == ended.sum() == int(eng.episode_count.item()) == len(mirror.records)
    _assert_same(got, mirror.records, f'{config} {flow} auto_reset={mode}')
    columns = dict(zip(R.COLUMNS, got.T))
    assert (columns['frames'] == columns['length']).all() and (columns['steps'] == columns['frames']).all() and (columns['length'] == CUT + 1).all()
    assert (columns['team'] == mirror.team).all() and set(columns['env']) == set(range(N_TILES)) and columns['episode'].min() >= 1
    assert np.isnan(columns['num_tracked']).all() == (team == 'target') and not np.isnan(columns['episode_reward']).any()
    assert seen_idle or (K == 1 and mode != 3)                  # idle frames (done = 2) were among the records read: behind an inner end, or waiting for the interval's restart


# ------------------------------------------------------------------ 2. everything finishes at once
def test_every_wave_appends_when_all_environments_finish_together():
    N = 80                                                     # five tiles: every wave a full ballot of four groups
    eng = _engine('MATE-4v8-9.yaml', N, cut=4)
    eng.enable_episode_records('target')
    mirror = Mirror(eng, 'target')
    for round_ in range(2):
        for _ in range(5):
            mirror.before()
            eng.step_random(auto_reset=True)
            torch.cuda.synchronize()
            mirror.frames(eng.scalars)
        got, dropped = _read(eng)
        assert dropped == 0 and len(got) == N and int(eng.episode_count.item()) == N * (round_ + 1)
        assert sorted(got[:, 0].tolist()) == list(range(N)) and (got[:, 1] == round_ + 1).all()      # none lost, none twice
        _assert_same(got, mirror.records[-N:], f'round {round_}')
    # ... and a last wave with a partial ballot: N = 70 leaves six groups in the last tile, a full wave and one of two
    eng = _engine('MATE-2v4-0.yaml', 70, cut=4)
    eng.enable_episode_records('camera')
    for _ in range(5):
        eng.step_random(auto_reset=True, want_masks=True)
    got, dropped = _read(eng)
    assert dropped == 0 and sorted(got[:, 0].tolist()) == list(range(70)) and not np.isnan(got[:, 14]).any()


# ------------------------------------------------------------------ 3. ring wrap
def test_ring_wrap_keeps_the_newest_records_in_their_slots():
    eng = _engine('MATE-2v4-0.yaml', N_TILES, cut=4)
    eng.enable_episode_records('target', capacity=8)
    mirror = Mirror(eng, 'target')
    for round_ in range(2):
        for _ in range(5):
            mirror.before()
            eng.step_random(auto_reset=True)
            torch.cuda.synchronize()
            mirror.frames(eng.scalars)
        total = int(eng.episode_count.item())
        assert total == N_TILES * (round_ + 1)
        got, dropped = _read(eng)
        assert len(got) == 8 and dropped == 25
        ring = eng.episode_ring.cpu().numpy()
        for i, n in enumerate(range(total - 8, total)):
            assert R.same_bits(ring[n % 8], got[i])              # slot n % capacity holds record n
        assert len(set(got[:, 0].tolist())) == 8 and (got[:, 1] == round_ + 1).all()
        expect = {row[0]: row for row in mirror.records[-N_TILES:]}
        for row in got:                                          # whole records of this round, none torn
            assert R.same_bits(row, expect[row[0]])
    got, dropped = _read(eng)
    assert len(got) == 0 and dropped == 0


# ------------------------------------------------------------------ 4. shaped rows and masks
SHAPING = ({'coverage_rate': 1.0, 'num_tracked': 0.25}, 'mean')


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_shaped_rows_and_masks(dtype):
    eng = _engine('MATE-4v8-9.yaml', N_TILES, policies=True)
    eng.enable_reward_rows(camera=SHAPING, dtype=dtype, terms=True)
    eng.enable_episode_records('camera')
    mirror = Mirror(eng, 'camera')
    gen = torch.Generator(device='cpu').manual_seed(4)
    for _ in range(2 * (CUT + 1)):
        mirror.before()
        eng.step_versus_greedy('camera', _random_actions(eng, gen)[0], auto_reset=True)
        torch.cuda.synchronize()
        mirror.frames(eng.scalars, eng.masks, rows=eng.camera_reward_rows, terms=eng.camera_reward_terms)      # the rows shaped_rewards() shows at this step
    got, dropped = _read(eng)
    assert len(got) == 2 * N_TILES
    _assert_same(got, mirror.records, str(dtype))
    assert not np.isnan(got[:, 7]).any() and not np.isnan(got[:, 14]).any()
    assert (got[:, 14] >= 0).all() and (got[:, 14] <= eng.num_targets).all()
    # the shaped row is not the team reward per agent: the column would differ
    assert not np.array_equal(got[:, 7], eng.num_cameras * got[:, 5])


def test_no_masks_gives_nan_tracked_and_accumulate_gives_nan_reward():
    eng = _engine('MATE-4v8-9.yaml', N_TILES, policies=True)
    eng.enable_episode_records('camera')
    mirror = Mirror(eng, 'camera')
    for _ in range(CUT + 1):
        mirror.before()
        eng.step_random(auto_reset=True, want_masks=False)
        torch.cuda.synchronize()
        mirror.frames(eng.scalars, None)
    got, _ = _read(eng)
    assert len(got) == N_TILES and np.isnan(got[:, 14]).all() and not np.isnan(got[:, 7]).any()
    _assert_same(got, mirror.records, 'no masks')
    assert np.array_equal(got[:, 7], eng.num_cameras * got[:, 5])      # RepeatedRewardIndividualDone: the team reward once per camera (exact: f32 terms)
    eng.enable_reward_rows(camera=SHAPING, accumulate=True, terms=True)
    gen = torch.Generator(device='cpu').manual_seed(4)
    for _ in range(CUT + 1):
        mirror.before()
        eng.step_versus_greedy('camera', _random_actions(eng, gen)[0], auto_reset=True)
        torch.cuda.synchronize()
        mirror.frames(eng.scalars, eng.masks, row_nan=True, terms=eng.camera_reward_terms)
    got, _ = _read(eng)
    assert len(got) == N_TILES and np.isnan(got[:, 7]).all() and not np.isnan(got[:, 14]).any()
    _assert_same(got, mirror.records[-N_TILES:], 'accumulate')


# ------------------------------------------------------------------ 5. the restated fragment form against the callback (the engine has the frame form only)
@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_fragments_against_the_callback(name):
    """The fixtures hold frames and fragments but no state to step from, and the episode launch runs behind stepping calls only: the
    fixture's frames go through the fragment launch on demand (as tests/test_gpu_fragment.py replays them), the contract's restatement
    runs over the engine's own fragment outputs, and its two records are held against the callback restated over the fixture's
    fragments.  Bound: every compared value comes from the scalar record, which is f32 whatever the observation type, so the bound
    is the project's f32 bar, 1e-5 * max(1, |ref|) (1e-9 absolute is the bar of f64 observation rows, which a record does not hold)."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    fx = G.load(name + '.npz')
    K, team = int(fx['frame_skip']), str(fx['learner_team'])
    frags = fragments_of(fx)
    F = len(frags)
    eng = Engine(read_config(str(fx['config_file'])), F, seed=1, obs_dtype=torch.float64)
    eng.reset()
    A, D = fx['frame/rows'].shape[1:]
    MW, W = eng.layout.mask_words, fx['frame/view_words'].shape[1]
    rows, scalars, masks = np.zeros((K, F, A, D)), np.zeros((K, F, 8), dtype=np.float32), np.zeros((K, F, MW), dtype=np.uint32)
    scalars[:, :, 2] = 2.0
    for n, (first, frames) in enumerate(frags):
        rows[:frames, n] = fx['frame/rows'][first:first + frames]
        scalars[:frames, n] = fx['frame/scalars'][first:first + frames].astype(np.float32)
        masks[:frames, n, :W] = fx['frame/view_words'][first:first + frames]
    dev = eng.device
    out = eng.fragment_rows(team, torch.from_numpy(rows).to(dev), torch.from_numpy(scalars).to(dev), torch.from_numpy(masks.view(np.int32)).to(dev))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    code, agents = (0, int(fx['num_cameras'])) if team == 'camera' else (1, int(fx['num_targets']))
    sums, collector, records, metrics = R.EpisodeSums(code, agents, int(fx['num_cameras'])), R.MetricCollector(), [], []
    for n in range(F):
        collector.add([dict(zip((str(k) for k in fx['info_names']), fx['skip/info'][n]))] * agents)
        if sums.fragment(got['frames'][n], got['done'][n], got['rewards'][n], got['info'][n]):
            records.append(dict(zip(R.COLUMNS, sums.record(0, len(records) + 1, 0))))
            metrics.append(collector.episode_end())
            collector = R.MetricCollector()
    assert len(records) == len(metrics) == 2
    for record, expect in zip(records, metrics):
        for key in ('raw_reward', 'normalized_raw_reward', 'coverage_rate', 'real_coverage_rate', 'mean_transport_rate', 'num_delivered_cargoes',
                    'episode_raw_reward', 'episode_normalized_raw_reward'):
            error, bound = abs(record[key] - expect[key]), 1e-5 * max(1.0, abs(expect[key]))
            print(f'{name} {key}: {record[key]!r} against {expect[key]!r}, error {error:.3e}, bound {bound:.3e}')
            assert error <= bound, key


# ------------------------------------------------------------------ 6. graph replay
@pytest.mark.parametrize('versus,frame_skip', [('camera', 1), ('target', 5)])
def test_graph_replay_gives_the_records_of_direct_calls(versus, frame_skip):
    config = 'MATE-4v8-9.yaml'
    cut = CUT if frame_skip == 1 else 11
    engines = []
    for _ in range(2):
        eng = _engine(config, N_TILES, cut=cut, policies=True, seed=9)
        eng.enable_episode_records(versus)
        engines.append(eng)
    a, b = engines                                               # graph-replayed | launched directly
    agents = a.num_cameras if versus == 'camera' else a.num_targets
    act = torch.zeros((N_TILES, agents, 2), dtype=torch.float64, device=a.device)
    act[:, :, 0] = 2.0
    cam_act, tgt_act = (act, None) if versus == 'camera' else (None, act)
    steps = 3 * (cut + 1) // frame_skip + 2
    steps -= steps % 2
    stepper = a.make_stepper(cam_act, tgt_act, auto_reset=1, graph_steps=2, versus=versus, frame_skip=frame_skip)      # built after enabling: the capture holds the launch
    stepper.run(steps)
    for _ in range(stepper.warmup_steps + steps):
        if frame_skip > 1:
            b.rollout_versus_greedy(versus, act, frame_skip, auto_reset=1)
        else:
            b.step_versus_greedy(versus, act, auto_reset=1)
    torch.cuda.synchronize()
    got_a, dropped_a = _read(a)
    got_b, dropped_b = _read(b)
    stepper.close()
    assert dropped_a == dropped_b == 0 and len(got_a) >= 2 * N_TILES
    _assert_same(got_a, got_b, f'versus={versus} frame_skip={frame_skip}')
    assert (got_a[:, 3] == got_a[:, 4]).all() and (got_a[:, 4] == cut + 1).all()


# ------------------------------------------------------------------ 7. episodes in progress
def test_masked_reset_discards_the_partial_sums_of_the_masked_environments():
    eng = _engine('MATE-2v4-0.yaml', N_TILES)
    eng.enable_episode_records('target')
    mirror = Mirror(eng, 'target')
    mask = torch.zeros(N_TILES, dtype=torch.bool, device=eng.device)
    mask[[0, 5, 16, 32]] = True
    for step in range(2 * (CUT + 1) + 4):
        if step == 4:                                            # halfway through the first episode
            eng.reset(mask)
            mirror.discard(mask.cpu().numpy())
        mirror.before()
        eng.step_random(auto_reset=True)
        torch.cuda.synchronize()
        mirror.frames(eng.scalars)
    got, _ = _read(eng)
    _assert_same(got, mirror.records, 'masked reset')
    assert int(eng.episode_count.item()) == len(mirror.records)          # no record for the discarded part
    got = R.sort_records(got)
    assert (got[:, 3] == got[:, 4]).all() and (got[:, 2] == CUT + 1).all()      # the masked environments' records start from zero at their reset
    first = {int(row[0]): row for row in got[::-1]}
    assert all(first[n][1] == 2 for n in (0, 5, 16, 32)) and first[1][1] == 1      # (the reset took episode number 2; nothing was recorded for 1)


def _run_random(eng, steps):
    for _ in range(steps):
        eng.step_random(auto_reset=True)
    return _read(eng)[0]


def test_seed_and_reset_reproduce_the_records():
    eng = _engine('MATE-4v2-9.yaml', N_TILES)
    eng.enable_episode_records('target')
    eng.seed(5)
    eng.reset()
    assert len(_run_random(eng, 4)) == 0                          # stopped inside episode 1 ...
    eng.seed(5)                                                   # ... whose number the next episode repeats: its partial sums must be gone
    eng.reset()
    first = _run_random(eng, CUT + 1 + 3)
    assert len(first) == N_TILES and (first[:, 3] == CUT + 1).all() and (first[:, 4] == CUT + 1).all() and (first[:, 1] == 1).all()
    eng.seed(5)
    eng.reset()
    again = _run_random(eng, CUT + 1 + 3)
    _assert_same(again, first, 'seed')


def test_import_state_gives_partial_records_first():
    eng = _engine('MATE-4v2-9.yaml', N_TILES)
    eng.enable_episode_records('target')
    for _ in range(4):
        eng.step_random(auto_reset=True)
    checkpoint = eng.export_state().clone()
    assert len(_run_random(eng, 6)) == N_TILES
    eng.import_state(checkpoint)
    got = R.sort_records(_run_random(eng, 4 + CUT + 1))
    assert len(got) == 2 * N_TILES
    first, later = got[0::2], got[1::2]
    assert (first[:, 3] == CUT + 1 - 4).all() and (first[:, 4] == CUT + 1).all() and (first[:, 3] < first[:, 4]).all()
    assert (later[:, 3] == later[:, 4]).all() and (later[:, 1] == first[:, 1] + 1).all()


# ------------------------------------------------------------------ 8. refusals leave the engine usable
def test_refusals_leave_the_engine_usable():
    from mate_amd._native import EngineError, check
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    eng = Engine(read_config('MATE-4v2-9.yaml', max_episode_steps=CUT), 8, seed=1)
    eng.enable_policies()
    with pytest.raises(EngineError, match='before reset') as info:
        eng.enable_episode_records('target')
    assert info.value.code == -4 and eng.episode_ring is None     # MATE_ESTATE
    eng.reset()
    nav = Engine(read_config('MATE-Navigation.yaml'), 8, seed=1)
    nav.reset()
    with pytest.raises(EngineError, match='no cameras') as info:
        nav.enable_episode_records('camera')
    assert info.value.code == -1 and nav.episode_ring is None     # MATE_EINVAL
    nav.enable_episode_records('target')
    nav.step_random()

    def refused(call, code, match):
        before = eng.export_state().clone()
        with pytest.raises(EngineError, match=match) as info:
            call()
        assert info.value.code == code
        assert torch.equal(eng.export_state(), before)

    buf = torch.zeros(64, dtype=torch.float64, device=eng.device)
    count = torch.zeros(1, dtype=torch.int64, device=eng.device)
    raw = lambda *args: (lambda: check(eng.lib.mate_engine_enable_episode_records(eng._h, *args)))      # noqa: E731
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)      # noqa: E731
    refused(raw(2, ptr(buf), 4, ptr(count)), -1, 'team')
    refused(raw(1, ptr(buf), 0, ptr(count)), -1, 'capacity')
    refused(raw(1, ptr(buf), 4, None), -1, 'counter')
    refused(raw(1, ptr(buf, 4), 3, ptr(count)), -1, 'aligned')
    eng.enable_fragment_rows('camera', 3)
    eng.enable_episode_records('camera')
    act = torch.zeros((8, eng.num_cameras, 2), dtype=torch.float64, device=eng.device)

    def without_scalars():
        io, keep = eng._io()
        io.scalars_dev = None
        check(eng.lib.mate_engine_step_random(eng._h, ctypes.byref(io), 1, eng._stream()))
    refused(without_scalars, -1, 'scalars_dev')
    refused(lambda: eng.rollout_greedy(2, auto_reset='pipelined'), -4, 'pipelined')
    eng.rollout_versus_greedy('camera', act, 3)                    # the next valid calls succeed: a fused call behind the fragment launch (its frames are the steps) ...
    eng.step_versus_greedy('camera', act)                          # ... and a per-step one
    for _ in range(CUT + 1 - 4):
        eng.step_random()
    got = _read(eng)[0]
    assert len(got) == 8 and (got[:, 2] == CUT + 1).all() and (got[:, 3] == got[:, 4]).all()
    eng.disable_fragment_rows()                                    # the records do not depend on the fragment rows
    assert eng.episode_ring is not None
    for _ in range(CUT + 1):
        eng.step_random()
    assert len(_read(eng)[0]) == 8


def test_detaching_restores_the_flows():
    engines = [_engine('MATE-4v8-9.yaml', N_TILES, policies=True, seed=6) for _ in range(2)]
    a, b = engines                                               # records enabled, used, detached | never enabled
    act = torch.zeros((N_TILES, a.num_cameras, 2), dtype=torch.float64, device=a.device)
    a.enable_episode_records('camera')
    for e in engines:
        e.step_versus_greedy('camera', act)
    a.disable_episode_records()
    assert a.episode_ring is None and a.episode_count is None
    for step in range(10):
        act[:, :, 0] = float(step)
        for e in engines:
            e.step_versus_greedy('camera', act)
        torch.cuda.synchronize()
        assert a.last_flow == b.last_flow
        for name in ('camera_obs', 'target_obs', 'scalars', 'masks'):
            assert torch.equal(getattr(a, name), getattr(b, name)), (step, name)
    assert torch.equal(a.export_state(), b.export_state())


# ------------------------------------------------------------------ 9. environment class and evaluate
def test_batched_environment_episodes():
    from mate_amd.environment import BatchedMultiAgentTracking
    env = BatchedMultiAgentTracking('MATE-4v2-9.yaml', num_envs=N_TILES, seed=4, episode_records=True, max_episode_steps=CUT)
    env.reset()
    assert env.engine.episode_team == 1                          # True without a learner: the target team's
    for _ in range(CUT + 1):
        env.step_random()
    out = env.episodes()
    assert set(out) == set(R.COLUMNS) | {'dropped'} and len(out) == 17 and out['dropped'] == 0
    assert all(out[name].shape == (N_TILES,) for name in R.COLUMNS) and bool((out['length'] == CUT + 1).all())
    env.close()
    env = BatchedMultiAgentTracking('MATE-4v2-9.yaml', num_envs=N_TILES, seed=4, episode_records=True, frame_skip=3, learner='camera', max_episode_steps=CUT)
    env.reset()
    assert env.engine.episode_team == 0                          # True with a learner: the learner's
    act = torch.zeros((N_TILES, env.num_cameras, 2), dtype=torch.float64, device=env.device)
    for _ in range(3):
        env.step_fragment(act)
    out = env.episodes()
    assert bool((out['steps'] == CUT + 1).all()) and bool((out['frames'] == CUT + 1).all())      # a fragment counts as its frames
    env.close()


def test_evaluate_reports_ten_columns_over_the_batch(capsys):
    from mate_amd import evaluate
    from mate_amd.engine import Engine
    records = evaluate.main(['--config', 'MATE-4v2-9.yaml', '--num-envs', '64', '--episodes', '64', '--policy', 'greedy', '--max-episode-steps', '15'])
    assert records.shape == (64, 16)
    lines = [line.strip() for line in capsys.readouterr().out.splitlines() if '+-' in line]
    assert [line.split(':')[0] for line in lines] == list(Engine.EPISODE_COLUMNS[5:15]) and len(lines) == 10
    values = {line.split(':')[0]: float(line.split(':')[1].split('+-')[0]) for line in lines}
    assert 0.0 <= values['coverage_rate'] <= 1.0
