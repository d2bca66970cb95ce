"""CPU: the host side of the Naive / Random opponents and the opponent mixtures (csrc/scripted_rows.hpp) -- the restatement of tests/scripted_ref.py
against NumPy's own RandomState.choice(p=) and against hand-worked cases of the reference's rules, the header, and the Python-level validation that needs no
device (the unit's resource record and the source digest: tests/test_unit_resources.py)."""
import os
import re

import numpy as np
import pytest

import golden_util as G
import scripted_ref as R

FIXTURES = ['naive_4v8-9', 'naive_2v4-0', 'naive_8v8-9', 'random_4v8-9', 'random_2v4-0']
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mixture_choice_is_random_state_choice():
    """mixture.py:108 draws np_random_mixture.choice(candidates, p=weights): one uniform of the same generator through the searchsorted rule picks the
    same candidate, zero weights removed first (mixture.py:41-43)."""
    for weights in ([1.0, 2.0, 1.0], [1.0, 3.0], [0.5, 0.0, 0.25, 0.25, 1.0], [7.0], [1e-3, 1.0, 1e-3]):
        w = np.asarray(weights)
        p = w[w > 0.0] / w[w > 0.0].sum()
        a, b = np.random.RandomState(12), np.random.RandomState(12)
        want = np.array([a.choice(len(p), p=p) for _ in range(2000)])
        got = R.mixture_choice(weights, b.random_sample(2000))
        assert np.array_equal(want, got), weights
        assert set(got.tolist()) == set(range(len(p))) or len(p) > 3
    # the rims: u equal to a cumulative sum belongs to the NEXT candidate (side='right'); rounding short of 1 stays on the last
    assert R.mixture_choice([1.0, 1.0], [0.0, 0.5 - 2 ** -54, 0.5, 1.0 - 2 ** -53]).tolist() == [0, 0, 1, 1]
    assert R.mixture_choice([0.1] * 10, [1.0 - 2 ** -53]).tolist() == [9]


def test_binomial_mapping_is_the_recording_proxys():
    """tests/golden/make_golden.py AgentRNG.binomial: u > 1 - p for p <= 0.5, u <= p above -- what the Greedy targets' device code does (policy_kernels.hpp)."""
    u = np.array([0.0, 0.04, 0.75, 0.7500001, 0.94, 0.95, 0.9500001, 0.999])
    assert R.binomial1(0.05, u).tolist() == [False, False, False, False, False, False, True, True]
    assert R.binomial1(0.75, u).tolist() == [True, True, True, False, False, False, False, False]


def test_naive_and_random_rules_on_worked_cases():
    """naive.py:27, :79-105 and random.py:52-55 on cases small enough to follow by hand."""
    assert np.array_equal(R.naive_camera(np.array([0.0, 0.5, 1.0]), 5.0, 2.5), np.array([[0.0, 0.0], [1.0, 0.5], [2.0, 1.0]]))
    assert np.array_equal(R.box_sample(np.array([0.0, 0.25, 1.0]), 20.0), np.array([-20.0, -10.0, 20.0]))
    # five targets inside warehouse 0, goal 0: (a) carries: one increment; (b) unloaded, knows nothing empty: the loop form, whose first
    # test passes; (c) unloaded, knows 1 and 2 empty, inc +1: skips to 3; (d) the same with inc -1: 3 at once; (e) every warehouse empty: one increment
    xy = np.tile(R.WAREHOUSES[0] - [10.0, 20.0], (5, 1))
    mem = dict(goal=np.zeros(5, dtype=np.int64), inc=np.array([1, 1, 1, -1, 1]), prev_location=xy.copy(), prev_noise=np.full((5, 2), 0.5))
    carries = np.array([True, False, False, False, False])
    empty = np.array([0, 0, 0b0110, 0b0110, 0b1111])
    u = np.tile([0.9, 0.5, 0.5], (5, 1))      # stood still: prob 0.75, u = 0.9 keeps the noise
    out, new, info = R.naive_target_act(mem, xy, np.full(5, 20.0), carries, empty, u)
    assert new['goal'].tolist() == [1, 1, 3, 3, 1]
    assert info['once'].tolist() == [True, False, False, False, True] and info['skip'].tolist() == [False, True, True, True, False]
    assert info['skipped'].tolist() == [0, 0, 2, 0, 0] and not info['resample'].any() and (info['prob'] == 0.75).all()
    want = R.WAREHOUSES[new['goal']] - xy
    want = want * (20.0 / np.linalg.norm(want, axis=-1))[:, None]
    assert np.allclose(out, np.clip(want + 0.5, -20.0, 20.0), rtol=0, atol=1e-12)
    # outside 0.9 radius nothing advances; a moving target (prob 0.05) resamples on u > 0.95 only
    far = R.WAREHOUSES[0] - [0.0, 67.6]
    mem1 = dict(goal=np.zeros(2, dtype=np.int64), inc=np.ones(2, dtype=np.int64), prev_location=np.tile(far - [10.0, 0.0], (2, 1)), prev_noise=np.zeros((2, 2)))
    out, new, info = R.naive_target_act(mem1, np.tile(far, (2, 1)), np.full(2, 20.0), np.zeros(2, bool), np.zeros(2, int), np.array([[0.9, 1.0, 0.0], [0.96, 1.0, 0.0]]))
    assert new['goal'].tolist() == [0, 0] and (info['prob'] == 0.05).all() and info['resample'].tolist() == [False, True]
    assert np.array_equal(new['prev_noise'], np.array([[0.0, 0.0], [10.0, -10.0]]))
    # the Random agents' hold: a draw at calls 0, 3, 6 of an episode and at the first call of the next
    team = R.ScriptedTeam(0, 1, 2, frame_skip=3)
    high = np.broadcast_to(np.array([5.0, 2.5]), (1, 2, 2))
    drawn = []
    for call in range(8):
        episode = np.array([1 if call < 7 else 2])
        u = np.full((1, 2, 2), 0.1 * (call + 1))
        out = team.step(np.array([True]), episode, np.array([R.RANDOM]), {}, high, dict(u=u))
        drawn.append(bool(out['used_u'].all()))
        assert out['used_u'].all() or not out['used_u'].any()
    assert drawn == [True, False, False, True, False, False, True, True]
    assert np.array_equal(out['final'][0, 0], R.box_sample(np.array([0.8, 0.8]), np.array([5.0, 2.5])))


def test_sources_are_in_the_digest_and_the_header_declares_the_calls():
    """(The digest: tests/test_unit_resources.py.)"""
    from mate_amd import _native
    with open(os.path.join(ROOT, 'include', 'mate_engine.h')) as fh:
        header = fh.read()
    assert re.search(r'#define\s+MATE_ABI_VERSION\s+1\b', header)
    assert re.search(r'MATE_SCRIPTED_GREEDY = 0, MATE_SCRIPTED_HEURISTIC = 1, MATE_SCRIPTED_NAIVE = 2, MATE_SCRIPTED_RANDOM = 3, MATE_SCRIPTED_EXTERNAL = 4', header)
    assert re.search(r'enum \{ MATE_OPPONENT_GREEDY = 0, MATE_OPPONENT_HEURISTIC = 1 \};', header)      # the plain selections keep their two values
    for call in ('set_opponent_mixture', 'scripted_tape', 'scripted_memory', 'scripted_external', 'scripted_rows'):
        assert 'mate_engine_' + call in _native.PROTOTYPES
    with open(os.path.join(ROOT, 'mate_amd', 'csrc', 'scripted_rows.hpp')) as fh:
        streams = dict(re.findall(r'(S_SCR_\w+) = (\d+)', fh.read()))
    assert sorted(int(v) for v in streams.values()) == [22, 23, 24, 25]      # behind S_POL_* = 16..19 and S_HCAM_* = 20, 21


def test_python_level_validation_needs_no_device():
    from mate_amd.engine import CAMERA_AGENTS, SCRIPTED_AGENTS, TARGET_AGENTS, mixture_table
    from mate_amd.evaluate import build_parser, parse_mixture
    assert SCRIPTED_AGENTS == ('greedy', 'heuristic', 'naive', 'random', 'external') == R.SCRIPTED_AGENTS
    assert TARGET_AGENTS == CAMERA_AGENTS == ('greedy', 'heuristic')
    assert mixture_table('naive') == ([2], [1.0])
    assert mixture_table({'greedy': 1, 'random': 3}) == ([0, 3], [1.0, 3.0])
    assert mixture_table(['random', 'external'], [0, 2], random_frame_skip=1) == ([3, 4], [0.0, 2.0])
    for bad in (lambda: mixture_table('greedy2'), lambda: mixture_table(['naive', 'naive']), lambda: mixture_table([]),
                lambda: mixture_table(['naive', 'random'], [1.0]), lambda: mixture_table(['naive', 'random'], [1.0, -1.0]),
                lambda: mixture_table(['naive', 'random'], [0.0, 0.0]), lambda: mixture_table(['naive'], [float('nan')]),
                lambda: mixture_table(['naive'], [float('inf')]), lambda: mixture_table({'naive': 1.0}, [1.0]),
                lambda: mixture_table('naive', random_frame_skip=0), lambda: mixture_table('naive', random_frame_skip=2.5)):
        with pytest.raises(ValueError):
            bad()
    assert parse_mixture('naive') == {'naive': 1.0} and parse_mixture('greedy:1,random:1') == {'greedy': 1.0, 'random': 1.0}
    for bad in ('naive,naive', 'external', 'greedy:-1', 'fast'):
        with pytest.raises(ValueError):
            parse_mixture(bad)
    args = build_parser().parse_args(['--num-envs', '8', '--target-mixture', 'naive', '--episodes', '2'])
    assert args.target_mixture == {'naive': 1.0} and args.camera_mixture is None and args.target_agent == 'greedy'
    with pytest.raises(SystemExit):
        build_parser().parse_args(['--target-agent', 'naive'])      # the plain choices stay as they were


def test_environment_arguments_are_checked_ahead_of_the_device():
    from mate_amd.environment import BatchedMultiAgentTracking
    for kw in (dict(target_mixture='fast'), dict(camera_mixture={'naive': -1.0}), dict(target_mixture='naive', target_agent='heuristic'),
               dict(camera_mixture='naive', camera_selection='multi'), dict(target_mixture='naive', frame_skip=4, learner='camera')):
        with pytest.raises((ValueError, AssertionError)):
            BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=2, **kw)


@pytest.mark.parametrize('name', FIXTURES)
def test_restatement_equals_the_recorded_reference(name):
    """tests/golden/make_scripted_golden.py recorded the reference's Naive and Random pairs; the restatement reproduces every action to 1e-9 with no
    branch condition within 1e-9 of equality -- and the Naive cameras and both Random agents, which have no branches, bit for bit."""
    fx = G.load(name + '.npz')
    got = R.replay_fixture(fx)
    assert got['worst'] < 1e-9 and got['margin'] > 1e-9, (got['worst'], got['margin'])
    assert np.array_equal(got['cam'], fx['step/cam_act'])
    if name.startswith('random'):
        assert np.array_equal(got['tgt'], fx['step/tgt_act'])
        drawn = np.isfinite(fx['step/agent_tgt_sample_u']).all(axis=(1, 2))
        assert np.flatnonzero(drawn).tolist() == [0, 20, 40, 60] and len(drawn) == 70      # the hold is visible on both sides of every draw
        assert np.array_equal(fx['step/tgt_act'][19], fx['step/tgt_act'][0]) and not np.array_equal(fx['step/tgt_act'][20], fx['step/tgt_act'][19])
    if name == 'naive_4v8-9':        # the planted scene (remaining_cargoes[1] and [2] emptied) shows every branch of the arrival rule and of the noise rule
        assert got['once'] > 0 and got['skip'] > 0 and got['far'] > 0 and got['p05'] > 0 and got['p75'] > 0, got
        assert len(fx['step/done']) == 500


def test_searchsorted_rule_and_restatement_against_the_recorded_mixture():
    """mixture_4v8-9.npz: the reference's MixtureTargetAgent([Greedy, Naive, Random], [1, 2, 1]) through 8 episodes of one environment -- every agent of
    the team draws the same candidate (spawn() seeds them alike), the uniform its choice(p=) consumed gives that candidate through the searchsorted
    rule, all three candidates play, and the restatement reproduces the actions of every Naive and Random episode to 1e-9 (the Random ones bit for bit)."""
    fx = G.load('mixture_4v8-9.npz')
    names = [str(c) for c in fx['candidates']]
    played = []
    for ep in R.mixture_episodes(fx):
        assert ep['choice'].shape == (8,) and (ep['choice'] == ep['choice'][0]).all()
        assert np.array_equal(R.mixture_choice(fx['weights'], ep['uniform']), ep['choice'])
        assert str(ep['policy']) == names[int(ep['choice'][0])] and len(ep['step/done']) == 12
        played.append(str(ep['policy']))
        if played[-1] != 'greedy':
            got = R.replay_fixture(ep, teams=(1,))
            assert got['worst'] < 1e-9 and got['margin'] > 1e-9, (played, got['worst'], got['margin'])
            assert played[-1] != 'random' or np.array_equal(got['tgt'], ep['step/tgt_act'])
    assert len(played) == 8 and set(played) == set(names)
