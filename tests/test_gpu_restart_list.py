"""GPU (-m gpu): THE RESTART-LIST PROTOCOL, as every stepping kernel has to follow it (csrc/engine_kernels.hpp, "The restart list").

Six environments -- ragged against the four environments of a workgroup and against every sub-wave group size -- with episodes
of max_episode_steps = 2, through each stepping entry point.  Every expected value follows from the protocol; there is no golden:

1. auto_reset = 0 until every environment has reported done == 1: nobody keeps a list, the records say "finished" (1).
2. Two steps of a batched interval (auto_reset = 3): the finished environments idle -- row (0, 0, 2, 0, 0, 0, 0, 0), one
   idle step each per step -- and the first of the two lists them late and marks the records "listed" (3; the fused rollouts
   restart an interval by flag, keep no list and leave the records at 1).
3. The interval's third call: they idle once more and restart behind it -- every one of them, once: `done` 0, episode step 0,
   the episode counter one up.
4. A whole second interval of live environments: nobody idles, the episodes end on its last call and restart behind it
   (an entry left on either list would have restarted somebody in the middle of an episode).
5. Finished under auto_reset = 0 once more, then ONE call with auto_reset = 1: listed by that call (at its entry, on its idle
   path, or by the step a per-step flow without a pending interval takes), restarted behind it.

The engines of set_sub_wave(False) and set_sub_wave(True) run side by side and agree bit for bit behind every call.  The `step`
column runs once more under each switch of the launch matrix, which reaches the two-wave step and the per-step rollout form."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import launch_matrix as M  # noqa: E402
import shape_edges  # noqa: E402
from mate_amd.config import read_config  # noqa: E402
from mate_amd.engine import Engine, export_layout  # noqa: E402

pytestmark = pytest.mark.gpu

N = 6
INTERVAL = 3
SHAPES = ('MATE-2v4-0', '3v5-7')
ENTRY_POINTS = ('step', 'step_random', 'step_greedy', 'step_versus_greedy', 'rollout_random', 'rollout_greedy')
IDLE_ROW = torch.tensor([0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0])


def same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def config_of(shape):
    if shape.startswith('MATE-'):
        return read_config(shape + '.yaml', max_episode_steps=2)
    return read_config(dict(shape_edges.scenario((3, 5, 7)), max_episode_steps=2))


class Pair:
    """The engines of set_sub_wave(False) and set_sub_wave(True), stepped together."""

    def __init__(self, shape):
        self.engines = []
        for mode in (False, True):
            eng = Engine(config_of(shape), N, seed=11, first_env_index=2)
            eng.set_sub_wave(mode)
            eng.enable_policies()
            eng.reset()
            eng.reserve_rollout(4, want_masks=True, search='none')
            self.engines.append(eng)
        self.acts = M.actions_of(self.engines[0])
        layout, _ = export_layout(eng.num_cameras, eng.num_targets, eng.num_obstacles)
        self.word = {name: layout[name][0] for name in ('episode_step', 'episode', 'done')}

    def issue(self, eng, entry, auto_reset, steps):
        cam, tgt, _ = self.acts
        if entry == 'step':
            return eng.step(cam, tgt, auto_reset=auto_reset)
        if entry == 'step_random':
            return eng.step_random(auto_reset=auto_reset, want_masks=True)
        if entry == 'step_greedy':
            return eng.step_greedy(auto_reset=auto_reset)
        if entry == 'step_versus_greedy':
            return eng.step_versus_greedy('camera', cam, auto_reset=auto_reset)
        if entry == 'rollout_random':
            return eng.rollout_random(steps, auto_reset=auto_reset, want_masks=True)
        assert entry == 'rollout_greedy', entry
        return eng.rollout_greedy(steps, auto_reset=auto_reset, want_masks=True)

    def call(self, entry, auto_reset, steps=1):
        """One call on both engines, held to the same bits (outputs, both mask buffers, the records, as tests/test_gpu_launch_matrix.py
        does); returns the scalar rows [steps, N, 8] on the host."""
        one, sub = self.engines
        out_one, out_sub = (self.issue(eng, entry, auto_reset, steps) for eng in self.engines)
        what = (entry, auto_reset, steps)
        for x, y in zip(out_one, out_sub):
            assert same(x, y), what
        assert same(one.masks, sub.masks) and same(one._rollout['masks'], sub._rollout['masks']), what
        assert same(one.export_state(), sub.export_state()), what
        rows = out_one[2].float().cpu()
        return rows if rows.dim() == 3 else rows[None]

    def state(self, name):
        return self.engines[0].export_state()[:, self.word[name]].cpu().long()

    def idle(self):
        counts = [eng.idle_steps() for eng in self.engines]
        assert counts[0] == counts[1]
        return counts[0]

    def close(self):
        for eng in self.engines:
            eng.close()


def finish_everybody(pair, entry, steps):
    """auto_reset = 0 until every environment has reported done == 1 once."""
    reported = torch.zeros(N, dtype=torch.bool)
    for _ in range(4):
        reported |= (pair.call(entry, 0, steps)[:, :, 2] == 1.0).any(dim=0)
        if bool(reported.all()):
            break
    assert bool(reported.all()), reported
    done = pair.state('done')
    assert bool((done == 1).all()), done       # finished, on no list: nobody kept one


def run_protocol(entry):
    rollout = entry.startswith('rollout')
    steps = 4 if rollout else 1
    for shape in SHAPES:
        pair = Pair(shape)
        try:
            finish_everybody(pair, entry, steps)
            episode = pair.state('episode')
            # 2. two idle steps of a batched interval
            idle = pair.idle()
            for _ in range(2):
                rows = pair.call(entry, INTERVAL, 1)
                assert rows.shape == (1, N, 8) and bool((rows == IDLE_ROW).all()), rows
                # listed late by the first of the two and marked in the record; a fused rollout's interval restarts by flag: no list, still "finished"
                assert bool((pair.state('done') == (1 if rollout else 3)).all()), pair.state('done')
            assert pair.idle() - idle == N * 2
            assert bool((pair.state('episode') == episode).all())
            # 3. the interval's last call: idle once more (every row of it), restarted behind it
            idle = pair.idle()
            rows = pair.call(entry, INTERVAL, steps)
            assert bool((rows == IDLE_ROW).all()), rows
            assert pair.idle() - idle == N * steps
            assert bool((pair.state('done') == 0).all()) and bool((pair.state('episode_step') == 0).all())
            assert bool((pair.state('episode') == episode + 1).all())       # restarted once
            # 4. a second interval, everybody live: ends with the episodes (three steps each) and restarts them
            idle = pair.idle()
            if rollout:          # (three launches: one step, one step, then the step that ends the episodes and three idle ones)
                for k in range(INTERVAL):
                    rows = pair.call(entry, INTERVAL, 1 if k < 2 else steps)
                    assert bool((rows[0, :, 2] == (1.0 if k == 2 else 0.0)).all()), (k, rows)
                    assert bool((rows[1:] == IDLE_ROW).all()), (k, rows)
                    if k < 2:
                        assert bool((pair.state('episode_step') == k + 1).all()) and bool((pair.state('episode') == episode + 1).all())
                assert pair.idle() - idle == N * (steps - 1)
            else:
                for k in range(INTERVAL):
                    rows = pair.call(entry, INTERVAL, 1)
                    assert bool((rows[0, :, 2] == (1.0 if k == 2 else 0.0)).all()), (k, rows)
                    if k < 2:
                        assert bool((pair.state('episode_step') == k + 1).all()) and bool((pair.state('episode') == episode + 1).all())
                assert pair.idle() == idle
            assert bool((pair.state('done') == 0).all()) and bool((pair.state('episode_step') == 0).all())
            assert bool((pair.state('episode') == episode + 2).all())
            # 5. finished under auto_reset = 0 again; one call with auto_reset = 1 lists and restarts everybody
            finish_everybody(pair, entry, steps)
            rows = pair.call(entry, 1, steps)
            if entry in ('step', 'step_random'):      # (no interval pending: a finished environment steps, and that step lists it)
                assert bool((rows[:, :, 2] == 1.0).all()), rows
            else:
                assert bool((rows == IDLE_ROW).all()), rows
            assert bool((pair.state('done') == 0).all()) and bool((pair.state('episode_step') == 0).all())
            assert bool((pair.state('episode') == episode + 3).all())
            # ... and the call behind it finds nothing on either list: the new episodes take their first step
            rows = pair.call(entry, 1, 1)
            assert bool((rows[0, :, 2] == 0.0).all()), rows
            assert bool((pair.state('episode_step') == 1).all()) and bool((pair.state('episode') == episode + 3).all())
            torch.cuda.synchronize()
        finally:
            pair.close()


@pytest.mark.parametrize('entry', ENTRY_POINTS)
def test_finished_environments_idle_are_listed_once_and_restart(entry):
    run_protocol(entry)


@pytest.mark.parametrize('switch', M.SWITCH_COLUMNS)
def test_the_step_column_under_the_environment_switches(switch, monkeypatch):
    monkeypatch.setenv(*switch.split('='))        # (read by mate_engine_create)
    run_protocol('step')
