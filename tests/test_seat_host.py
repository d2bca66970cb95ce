"""Host-side tests of the learner's seat among on-device teammates (csrc/seat_rows.hpp), no GPU: the NumPy agents of tests/seat_ref.py against what the
reference's own SingleCamera / SingleTarget recorded (tests/golden/seat_*.npz, tests/golden/make_seat_golden.py) and, with nobody absent, against the oracle's
restatement of the agents, closed loop; the DRAW formula; the Python-level argument rules; the C ABI's prototypes and what of the refusal table needs no device."""
import os
import re

import numpy as np
import pytest

import golden_util as G
import seat_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = {      # name -> (team, seat, shuffle_entities)
    'seat_camera_4v8-9': ('camera', 3, False), 'seat_camera_8v8-9_shuffle': ('camera', 4, True),
    'seat_target_4v8-9': ('target', 7, False), 'seat_target_4v8-9_fewcargo': ('target', 7, False),
}


@pytest.mark.parametrize('name', sorted(FIXTURES))
def test_seat_ref_equals_the_recorded_reference(name):
    """Every recorded step: the teammates' and the opponents' actions to 1e-9, a delay drawn exactly for the pairs the reference drew one for (the seat's row
    none, the seat's column its one 'state' message per teammate); the joint action the environment consumed holds the learner's action in the seat's row;
    the wrapper returned the seat's row.  The coverage the recorder accepted the seed for is there."""
    fx = G.load(name + '.npz')
    team, seat, shuffle = FIXTURES[name]
    assert (str(fx['seat/team']), int(fx['seat/index']), bool(fx['seat/shuffle'])) == (team, seat, shuffle)
    n = int(fx['num_cameras'] if team == 'camera' else fx['num_targets'])
    assert 0 < seat < n - 1 if shuffle else seat == n - 1
    worst, total = S.replay(fx)
    assert worst < 1e-9, worst
    T = len(fx['step/done'])
    assert T >= 60
    acts = fx['step/cam_act' if team == 'camera' else 'step/tgt_act']
    assert np.array_equal(acts[:, seat], fx['step/seat_action'])
    prefix = 'cam' if team == 'camera' else 'tgt'
    assert np.isnan(fx[f'step/agent_{prefix}_binom_u'][:, seat]).all() and np.isnan(fx[f'step/agent_{prefix}_sample_u'][:, seat]).all()      # the seat draws nothing
    if team == 'camera':
        delay = fx['step/agent_cam_delay']
        assert (delay[:, seat, :] == -1).all()                              # ... and sends nothing
        assert ((delay[:, :, seat] >= 0).sum(axis=0) == np.where(np.arange(n) == seat, 0, 1)).all()      # every teammate's one 'state' message, never again
        assert total['state_to_seat'] == n - 1 and total['told'] >= 1
        assert (delay[:, np.arange(n) != seat][:, :, np.arange(n) != seat] >= 0).sum() > 2 * (n - 1) * (n - 2)      # second sends among the teammates occur
    else:
        assert np.isnan(fx['step/agent_tgt_choice_u'][:, seat]).all()
    if name.endswith('fewcargo'):
        assert total['broadcasts'] >= 1
    assert fx['step/seat_obs'].shape == (T, fx['reset/seat_obs'].shape[0])
    for key in fx:
        assert fx[key].dtype.kind in 'fiubU', key                           # arrays and names only
    assert os.path.getsize(os.path.join(G.GOLDEN_DIR, name + '.npz')) < 1 << 20


@pytest.mark.parametrize('config,steps', [('MATE-4v8-9.yaml', 64), ('MATE-8v8-9.yaml', 64)])
def test_seat_ref_without_a_seat_is_the_oracle_restatement(config, steps, oracle_lib):
    """Nobody absent: seat_ref equals oracle.GreedyPolicies.act, closed loop on the oracle environment with random tapes, to 1e-12 at every step.  (The
    oracle's agents expose no memory; the integer memory decides every branch, so 64 closed-loop steps of equal actions hold it together.)"""
    O = oracle_lib
    import gpu_util as U
    from mate_amd.config import read_config
    cfg = read_config(config)
    batch = O.OracleBatch(U.oracle_proto_from_config(cfg, O), 3, seed=31, first_env_index=7)
    batch.reset(threads=1)
    rng = np.random.RandomState(12)
    worst = 0.0
    for e in range(3):
        env = batch.env(e)
        env.build_luts()
        Nc, Nt = env.Nc, env.Nt
        theirs, mine = O.GreedyPolicies(), S.SeatAgents(Nc, Nt)
        reset_u = rng.random_sample((Nt, 2))
        sent = 0
        for s in range(steps):
            t = (rng.random_sample(Nc), rng.random_sample((Nc, 2)), rng.randint(6, 50, size=(Nc, Nc)).astype(np.int32), rng.random_sample(Nt),
                 rng.random_sample(Nt), rng.random_sample((Nt, 2)), reset_u)
            ca, ta, info = mine.act(S.view_of_oracle(env), *t)
            ra, rt = theirs.act(env, *t)
            worst = max(worst, float(np.abs(ca - ra).max()), float(np.abs(ta - rt).max()))
            assert worst < 1e-12, (e, s, worst)
            sent += int(info['sent'].sum())
            env.step(ra, rt, rng.random_sample((Nc, Nt)), rng.random_sample(Nt))
        assert sent > Nc * (Nc - 1)                                          # second sends occurred


def test_draw_formula_against_the_oracle_philox(oracle_lib):
    """(uint64(philox(seed, env, episode, 27, team).x) * n) >> 32 lies in [0, n), is 0 for n = 1, and visits every seat."""
    O = oracle_lib
    seed = 0x1234567890abcdef
    for n in (1, 2, 4, 8, 16):
        seen = set()
        for env in range(40):
            for episode in (1, 2, 3):
                for team in (0, 1):
                    x = O.philox(seed & 0xffffffff, seed >> 32, 1000 + env, episode, 27, team)[0]
                    z = S.seat_draw(seed, 1000 + env, episode, team, n, O.philox)
                    assert 0 <= z < n and z == int(np.uint64(x) * np.uint64(n) >> np.uint64(32)) == int(x * n // 2 ** 32)
                    seen.add(z)
        assert seen == set(range(n)), n
    with open(os.path.join(ROOT, 'mate_amd', 'csrc', 'seat_rows.hpp')) as fh:
        text = fh.read()
    streams = [int(v) for v in re.findall(r'S_SEAT\w* = (\d+)', text)]
    taken = []
    for unit in ('device_math.hpp', 'policy_kernels.hpp', 'opponent_rows.hpp', 'scripted_rows.hpp', 'channel_rows.hpp'):
        with open(os.path.join(ROOT, 'mate_amd', 'csrc', unit)) as fh:
            taken += [int(v) for v in re.findall(r'\bS_[A-Z_]+ = (\d+)', fh.read())]
    assert streams == [27] and 27 not in taken and max(taken) == 26          # a stream id no other draw uses


def test_python_level_argument_rules_need_no_device():
    import torch
    from mate_amd.engine import seat_mode_of
    from mate_amd.evaluate import build_parser
    assert seat_mode_of('auto', False) == ('fixed', -1, None) and seat_mode_of('auto', True) == ('draw', 0, None) and seat_mode_of('draw', False) == ('draw', 0, None)
    assert seat_mode_of(0, True) == ('fixed', 0, None) and seat_mode_of(np.int64(5), False) == ('fixed', 5, None)
    tape = torch.zeros(4, dtype=torch.int32)
    assert seat_mode_of(tape, False)[0] == 'tape' and seat_mode_of(tape, False)[2] is tape
    for bad in ('first', -1, 1.5, True, None):
        with pytest.raises(ValueError):
            seat_mode_of(bad, False)
    args = build_parser().parse_args([])
    assert args.single_agent is None
    assert build_parser().parse_args(['--num-envs', '8', '--single-agent', 'camera']).single_agent == 'camera'
    with pytest.raises(SystemExit):
        build_parser().parse_args(['--single-agent', 'both'])


def test_environment_arguments_are_checked_ahead_of_the_device():
    from mate_amd.environment import BatchedMultiAgentTracking
    for kw in (dict(single_agent='both'), dict(single_agent='camera', seat='last'), dict(single_agent='camera', camera_agent='heuristic'),
               dict(single_agent='target', target_mixture={'greedy': 1.0, 'naive': 1.0}), dict(single_agent='camera', no_communication='camera'),
               dict(single_agent='target', message_dropout=0.3), dict(single_agent='camera', frame_skip=4, learner='camera'), dict(seat=2)):
        with pytest.raises((ValueError, AssertionError)):
            BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=2, **kw)


def test_sources_are_in_the_digest_and_the_header_declares_the_calls():
    """(The digest: tests/test_unit_resources.py.)"""
    from mate_amd import _native
    with open(os.path.join(ROOT, 'include', 'mate_engine.h')) as fh:
        header = fh.read()
    assert re.search(r'#define\s+MATE_ABI_VERSION\s+1\b', header)
    for call, arity in (('enable_seat', 8), ('step_seated', 5), ('seat_rows', 3)):
        assert re.search(r'\bint mate_engine_%s\(' % call, header)
        assert len(_native.PROTOTYPES['mate_engine_' + call][1]) == arity
        declared = re.search(r'\bint mate_engine_%s\(([^;]*)\);' % call, header).group(1)
        assert declared.count(',') == arity - 1, call
    assert [int(re.search(r'#define\s+MATE_SEAT_%s\s+(\d+)' % m, header).group(1)) for m in ('FIXED', 'DRAW', 'TAPE')] == [0, 1, 2]
    from mate_amd.engine import Engine
    assert Engine.SEAT_MODES == ('fixed', 'draw', 'tape')
    assert "learner's own messages are not provided" in header


def test_refusals_that_need_no_device():
    """The null-engine row of the refusal table, through ctypes (every other row needs an engine: tests/test_gpu_seat.py)."""
    from mate_amd import _native
    lib = _native.load()
    assert lib.mate_engine_enable_seat(None, 0, 0, 0, None, None, None, None) == -1         # MATE_EINVAL: null engine
    assert lib.mate_engine_step_seated(None, None, None, 1, None) == -1
    assert lib.mate_engine_seat_rows(None, None, None) == -1
    assert 'null engine' in lib.mate_engine_last_error().decode()
