"""GPU (-m gpu): the headline kernel's camera pass (csrc/headline_kernels.hpp: headline_camera_pass -- the cameras' draws and kinematics sixteen steps
at a time, lane l for camera l >> 4 at step l & 15, handed over step by step) against rollout_kernel, which steps the cameras one step at a time and
which the same engine runs with MATE_HEADLINE_UNIT=0.  Same seed, same calls: every output, the state, the idle count and the episode statistics byte
for byte; rows of idle slots are written by neither kernel and must keep the sentinel.  The cases are the ones a pass can get wrong: launch lengths
around sixteen, passes that start on either half of a Philox block, episodes that end inside a pass, and a state imported between two launches."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
LONGEST = 33


def _engine(headline, n, seed=47, **config):
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    os.environ['MATE_HEADLINE_UNIT'] = '1' if headline else '0'
    try:
        eng = Engine(read_config('MATE-4v8-9.yaml', **config), n, seed=seed, first_env_index=3, obs_dtype=torch.float32)
    finally:
        os.environ.pop('MATE_HEADLINE_UNIT', None)
    eng.reset()
    eng.reserve_rollout(LONGEST, want_masks=True)
    return eng


def _set_form(eng, shifted):
    from mate_amd._native import check
    check(eng.lib.mate_engine_set_store_form(eng._h, int(shifted)))


def _launch(eng, steps, auto_reset=True):
    """One fused launch into sentinel-filled buffers: [camera rows, target rows, scalars, masks] of the launch, then the engine's state behind it."""
    buf = eng.reserve_rollout(LONGEST, want_masks=True)
    buf['camera_obs'].fill_(SENTINEL); buf['target_obs'].fill_(SENTINEL); buf['masks'].fill_(-1)
    cam, tgt, sc = eng.rollout_random(steps, auto_reset=auto_reset, want_masks=True)
    torch.cuda.synchronize()
    assert eng.last_flow == 1 and eng.specialised
    return [cam.clone(), tgt.clone(), sc.clone(), buf['masks'][:steps].clone(), eng.export_state().clone(), torch.tensor([eng.idle_steps()]), eng.episode_stats.clone()]


def _same_bytes(x, y):
    return torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def _assert_same_launch(new, old):
    """-> (idle slots, episodes that ended) of the launch"""
    cam, tgt, sc, masks = new[:4]
    assert _same_bytes(sc, old[2])
    ran = sc[..., 2] != 2
    for x, y in ((cam, old[0]), (tgt, old[1])):
        assert _same_bytes(x[ran], y[ran])
        assert (x[~ran] == SENTINEL).all() and (y[~ran] == SENTINEL).all()
    assert _same_bytes(masks[ran], old[3][ran]) and (masks[~ran] == -1).all() and (old[3][~ran] == -1).all()
    for x, y in zip(new[4:], old[4:]):
        assert _same_bytes(x, y)
    return int((~ran).sum()), int((sc[..., 2] == 1).sum())


def _both(n, run, **config):
    """`run(engine)` -> list of launches, on the headline kernel and on rollout_kernel; -> (idle slots, ended episodes) over all of them"""
    runs = [run(_engine(headline, n, **config)) for headline in (True, False)]
    assert len(runs[0]) == len(runs[1]) > 0
    idle = ended = 0
    for new, old in zip(*runs):
        i, e = _assert_same_launch(new, old)
        idle, ended = idle + i, ended + e
    return idle, ended


@pytest.mark.parametrize('n', [5, 64])
def test_launch_lengths_around_a_pass_each_first_after_reset(n):
    """1, 15, 16, 17 and 33 steps: less than a pass, one short of it, exactly one, one more, two and one more -- each the first launch behind reset(),
    in both forms of the row stores."""
    def run(eng):
        rec = []
        for shifted in (0, 1):
            _set_form(eng, shifted)
            for steps in (1, 15, 16, 17, 33):
                eng.reset()
                rec.append(_launch(eng, steps))
        return rec
    _both(n, run)


@pytest.mark.parametrize('shifted', [0, 1])
@pytest.mark.parametrize('n', [5, 64])
def test_passes_that_start_on_odd_and_even_ticks(n, shifted):
    """Launches of 1, 16, 3 and 17 steps in a row start at ticks 0, 1, 17 and 20: a pass begins on the second half of a Philox block and on the first, and
    a block straddles two launches.  One more of 33 steps starts at tick 37: its second and third pass begin on odd ticks too, so a block also straddles
    two passes of ONE launch."""
    def run(eng):
        _set_form(eng, shifted)
        return [_launch(eng, steps) for steps in (1, 16, 3, 17, 33)]
    _both(n, run)


@pytest.mark.parametrize('auto_reset', [1, 2])
@pytest.mark.parametrize('max_episode_steps', [5, 16, 21])
@pytest.mark.parametrize('n', [5, 64])
def test_episodes_that_end_inside_a_pass(n, max_episode_steps, auto_reset):
    """Episodes of 5, 16 and 21 steps under launches of 16 and 33: an episode ends in the middle of a pass, on its last step, and in the second launch's first
    pass; the rest of the pass is never handed over.  Immediate restarts and the batched restart every second launch, both store forms; the launches
    that follow begin on restarted (and, batched, on still finished) environments."""
    def run(eng):
        rec = []
        for shifted in (0, 1):
            _set_form(eng, shifted)
            rec += [_launch(eng, steps, auto_reset=auto_reset) for steps in (16, 33, 16)]
        return rec
    idle, ended = _both(n, run, max_episode_steps=max_episode_steps)
    assert idle > 0 and ended >= n      # scalars[..., 2] held 2 (idle slots) and 1 (finished episodes)


@pytest.mark.parametrize('shifted', [0, 1])
@pytest.mark.parametrize('n', [5, 64])
def test_a_launch_after_an_imported_state(n, shifted):
    """A state exported behind a 5-step launch comes back behind a 7-step one (whose pass ran sixteen steps ahead and handed seven over): the next launch's
    pass starts from the record's angles."""
    def run(eng):
        _set_form(eng, shifted)
        rec = [_launch(eng, 5)]
        saved = eng.export_state().clone()
        rec.append(_launch(eng, 7))
        eng.import_state(saved)
        rec.append(_launch(eng, 17))
        assert _same_bytes(rec[0][4], saved) and not _same_bytes(rec[1][4], saved)
        return rec
    _both(n, run)
