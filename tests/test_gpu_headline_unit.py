"""GPU (-m gpu): headline_rollout_kernel (csrc/headline_kernels.hpp: the fused random-policy rollout of MATE-4v8-9 with f32 rows, compiled for that one
form in a translation unit of its own) against rollout_kernel, which the same engine runs with MATE_HEADLINE_UNIT=0 (read at create).  Same seed, same
calls: every output, the state, the idle count and the episode statistics byte for byte.  Observation and mask rows of a slot in which the environment
idled are written by neither kernel: they are left out of the comparison and must keep the sentinel they were filled with."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def _engine(headline, workload='MATE-4v8-9.yaml', n=64, seed=31, obs_dtype=torch.float32, **config):
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    os.environ['MATE_HEADLINE_UNIT'] = '1' if headline else '0'
    try:
        eng = Engine(read_config(workload, **config), n, seed=seed, first_env_index=7, obs_dtype=obs_dtype)
    finally:
        os.environ.pop('MATE_HEADLINE_UNIT', None)
    eng.reset()
    return eng


def _set_form(eng, shifted):
    from mate_amd._native import check
    check(eng.lib.mate_engine_set_store_form(eng._h, int(shifted)))


def _launch(eng, steps, auto_reset=True):
    """One fused launch into sentinel-filled buffers: [camera rows, target rows, scalars, masks] of the launch, then the engine's state behind it."""
    buf = eng.reserve_rollout(16, want_masks=True)
    buf['camera_obs'].fill_(SENTINEL); buf['target_obs'].fill_(SENTINEL); buf['masks'].fill_(-1)
    cam, tgt, sc = eng.rollout_random(steps, auto_reset=auto_reset, want_masks=True)
    torch.cuda.synchronize()
    assert eng.last_flow == 1 and eng.specialised
    return [cam.clone(), tgt.clone(), sc.clone(), buf['masks'][:steps].clone(), eng.export_state().clone(), torch.tensor([eng.idle_steps()]), eng.episode_stats.clone()]


def _same_bytes(x, y):
    return torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def _assert_same_launch(new, old):
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


@pytest.mark.parametrize('shifted', [0, 1])
@pytest.mark.parametrize('n', [5, 64])
def test_launches_of_one_two_and_seven_steps_in_a_row(n, shifted):
    """A partial workgroup (5) and sixteen whole ones; three launches in a row, of 1, 2 and 7 steps; both forms of the row stores."""
    runs = []
    for headline in (True, False):
        eng = _engine(headline, n=n)
        eng.reserve_rollout(16, want_masks=True)
        _set_form(eng, shifted)
        runs.append([_launch(eng, steps) for steps in (1, 2, 7)])
    for new, old in zip(*runs):
        _assert_same_launch(new, old)


def test_output_blocks_at_every_16_byte_offset_of_a_cache_line():
    """The row blocks' bases at each 16-byte offset inside a 128-byte line (views into one larger allocation): the shifted store form derives every row's
    shift, 0..7 chunks, from the base's offset and the row's index; the plain form stores where the base says."""
    n, steps = 5, 2
    runs = []
    for headline in (True, False):
        eng = _engine(headline, n=n)
        buf = eng.reserve_rollout(16, want_masks=True)      # (what _launch reserves: the views below stay bound)
        rec = []
        for shifted in (0, 1):
            _set_form(eng, shifted)
            for k in range(8):
                for key, chunk in (('camera_obs', k), ('target_obs', (k + 3) & 7)):
                    shape = buf[key].shape
                    numel = buf[key].numel()
                    pool = torch.full((numel + 64,), SENTINEL, dtype=torch.float32, device=buf[key].device)
                    first = (((-pool.data_ptr()) % 128) + 16 * chunk) // 4 % 32
                    view = pool[first:first + numel].view(shape)
                    assert (view.data_ptr() % 128) // 16 == chunk
                    buf[key] = view
                eng._forget_calls()
                rec.append(_launch(eng, steps))
        runs.append(rec)
    for new, old in zip(*runs):
        _assert_same_launch(new, old)


@pytest.mark.parametrize('auto_reset', [1, 3])
@pytest.mark.parametrize('n', [5, 64])
def test_episodes_that_end_inside_a_launch(n, auto_reset):
    """max_episode_steps = 5: every episode ends inside the first launch -- idle rows, the restart list (immediate restarts) or the batched restart
    (every third launch step), and launches that begin on restarted and on finished environments."""
    runs = []
    for headline in (True, False):
        eng = _engine(headline, n=n, max_episode_steps=5)
        runs.append([_launch(eng, steps, auto_reset=auto_reset) for steps in (7, 7, 2, 1, 7)])
    idle = ended = 0
    for new, old in zip(*runs):
        i, e = _assert_same_launch(new, old)
        idle, ended = idle + i, ended + e
    assert idle > 0 and ended >= n


def test_a_single_step_between_two_launches():
    """step_random() between two fused launches: the state the launch held in registers goes through the record, is stepped by step_kernel, and comes back."""
    runs = []
    for headline in (True, False):
        eng = _engine(headline, n=64, max_episode_steps=9)
        rec = [_launch(eng, 7)]
        eng.step_random(auto_reset=True, want_masks=True)
        torch.cuda.synchronize()
        single = [t.clone() for t in (eng.camera_obs, eng.target_obs, eng.scalars, eng.masks)]
        rec.append(_launch(eng, 7))
        runs.append((rec, single))
    for new, old in zip(runs[0][0], runs[1][0]):
        _assert_same_launch(new, old)
    for x, y in zip(runs[0][1], runs[1][1]):
        assert _same_bytes(x, y)


@pytest.mark.parametrize('workload,obs_dtype', [('MATE-4v8-0.yaml', torch.float32), ('MATE-4v8-9.yaml', torch.float64)])
def test_other_shapes_and_f64_rows_keep_their_kernels(workload, obs_dtype):
    """Another shape and an f64-observation engine of the headline's shape are not the headline's form: the switch changes nothing for them -- the same
    flow and specialisation reported, the same rows."""
    runs = []
    for headline in (True, False):
        eng = _engine(headline, workload=workload, n=64, obs_dtype=obs_dtype, max_episode_steps=5)
        rec = [_launch(eng, steps) for steps in (2, 7)]
        runs.append((rec, eng.last_flow, eng.specialised))
    assert runs[0][1:] == runs[1][1:] == (1, True)
    for new, old in zip(runs[0][0], runs[1][0]):
        _assert_same_launch(new, old)
