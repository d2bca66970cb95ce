"""GPU tests of the learner's seat among on-device teammates (csrc/seat_rows.hpp; Engine.enable_seat / step_seated / seat_rows): the reference's own
SingleCamera / SingleTarget recordings replayed (tests/golden/seat_*.npz), closed loops against tests/seat_ref.py on the oracle environment, a twin engine
fed the seat flow's rows through step_versus_greedy, the seat across episodes, graph replay, and what an enabled seat leaves alone."""
import numpy as np
import pytest
import torch

import golden_util as G
import gpu_util as U
import seat_ref as S
import shape_edges as E

pytestmark = pytest.mark.gpu

FIXTURES = ['seat_camera_4v8-9', 'seat_camera_8v8-9_shuffle', 'seat_target_4v8-9', 'seat_target_4v8-9_fewcargo']


def _view_tape(mask, n, dev):
    """See-through uniforms that reproduce a recorded view: u = 1 sees through, u = 0 goes to the occlusion test."""
    return torch.from_numpy(np.where(mask, 1.0, 0.0)[None].repeat(n, 0)).to(dev)


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_replay(name):
    """The reference's recording broadcast over 5 environments: joint actions (the learner's row included) within 1e-8, masks, goals and bounties exact,
    seat_obs the seat's row of the engine's own observations bit for bit, seat_index / seat_acted the recorded seat."""
    fx = G.load(name + '.npz')
    N = 5
    eng = U.engine_from_fixture(fx, N, obs_dtype=torch.float64)
    eng.enable_policies()
    team, z = str(fx['seat/team']), int(fx['seat/index'])
    camera = team == 'camera'
    seat_obs, seat_index, seat_acted = eng.enable_seat(team, z)
    dev = eng.device
    eng.observe(tape_ct=_view_tape(fx['reset/camera_target_view_mask'], N, dev))
    assert np.array_equal(eng.unpack_masks()['camera_target_view_mask'][0], fx['reset/camera_target_view_mask'])
    rows = eng.camera_obs if camera else eng.target_obs
    eng.seat_rows()
    assert torch.equal(seat_obs, rows[:, z]) and (seat_index == z).all()

    def bc(a, dtype=np.float64):
        a = np.asarray(a)
        return torch.from_numpy(np.broadcast_to(a, (N,) + a.shape).astype(dtype).copy()).to(dev)

    worst = 0.0
    for s in range(len(fx['step/done'])):
        tape = {'camera_resample_u': bc(np.nan_to_num(fx['step/agent_cam_binom_u'][s], nan=0.0)), 'camera_sample_u': bc(np.nan_to_num(fx['step/agent_cam_sample_u'][s], nan=0.0)),
                'camera_delay': bc(fx['step/agent_cam_delay'][s], np.int32), 'target_choice_u': bc(np.nan_to_num(fx['step/agent_tgt_choice_u'][s], nan=0.0)),
                'target_resample_u': bc(np.nan_to_num(fx['step/agent_tgt_binom_u'][s], nan=0.0)), 'target_sample_u': bc(np.nan_to_num(fx['step/agent_tgt_sample_u'][s], nan=0.0)),
                'target_reset_sample_u': bc(np.nan_to_num(fx['agent/tgt_reset_sample_u'], nan=0.0))}
        eng.step_seated(bc(fx['step/seat_action'][s]), policy_tape=tape, tape_ct=bc(np.nan_to_num(fx['step/tape_ct'][s], nan=0.0)),
                        tape_goal=bc(np.nan_to_num(fx['step/goal_u'][s], nan=0.0)), auto_reset=False)
        cam_act, tgt_act = (a.cpu().numpy() for a in eng.policy_actions())
        worst = max(worst, float(np.abs(cam_act - fx['step/cam_act'][s]).max()), float(np.abs(tgt_act - fx['step/tgt_act'][s]).max()))
        assert worst < 1e-8, (s, worst)
        assert np.array_equal((cam_act if camera else tgt_act)[:, z], np.broadcast_to(fx['step/seat_action'][s], (N, 2)))      # the learner's action, as given
        masks = eng.unpack_masks()
        assert np.array_equal(masks['camera_target_view_mask'][N - 1], fx['step/camera_target_view_mask'][s]), s
        sd = eng.state_dict()
        assert np.array_equal(sd['tgt_goals'][0], fx['step/tgt_goals'][s].astype(np.float64)), s
        assert np.array_equal(sd['bounties'][N - 1], fx['step/bounties'][s].astype(np.float64)), s
        assert torch.equal(seat_obs, rows[:, z]), s
        assert (seat_index == z).all() and (seat_acted == z).all()
        assert np.abs(seat_obs[2].cpu().numpy() - fx['step/seat_obs'][s]).max() < 1e-6, s      # ... and what the reference's wrapper returned


def _engine_and_oracle(O, cfg, n, seed, first, few_cargo=False):
    from mate_amd.engine import Engine
    eng = Engine(cfg, n, seed=seed, first_env_index=first, obs_dtype=torch.float32)
    eng.enable_policies()
    eng.reset()
    torch.cuda.synchronize()
    batch = O.OracleBatch(U.oracle_proto_from_config(cfg, O), n, seed=seed, first_env_index=first)
    batch.reset(threads=4)
    for e in range(n):
        for c in range(eng.num_cameras):
            batch.env(e).set_lut(c, *eng.lut_read(e, c))
    if few_cargo:                                   # only the cargoes in transit are left, in the oracle and on the device
        sd = eng.state_dict()
        remaining, awaiting = sd['remaining_cargoes'].copy(), sd['awaiting_cargo_counts'].copy()
        for e in range(n):
            env = batch.env(e)
            remaining[e], awaiting[e] = S.few_cargoes(env.get('remaining_cargoes'), env.get('tgt_goal_bits'), env.get('tgt_goals'))
            env.set('remaining_cargoes', remaining[e])
            env.set('awaiting_cargo_counts', awaiting[e])
        view = batch.gather('camera_target_view_mask').reshape(n, eng.num_cameras, eng.num_targets) != 0
        eng.load_state_dict({'remaining_cargoes': remaining, 'awaiting_cargo_counts': awaiting})
        eng.observe(tape_ct=torch.from_numpy(np.where(view, 1.0, 0.0)).to(eng.device))
        assert np.array_equal(eng.unpack_masks()['camera_target_view_mask'], view)
    return eng, batch


def _device_step(eng, auto_reset=False):
    dev = eng.device

    def step(tape, action, tape_ct, goal_u):
        eng.step_seated(torch.from_numpy(action).to(dev), policy_tape={k: torch.from_numpy(v).to(dev) for k, v in tape.items()},
                        tape_ct=torch.from_numpy(tape_ct).to(dev), tape_goal=torch.from_numpy(goal_u).to(dev), auto_reset=auto_reset)
        return tuple(a.cpu().numpy() for a in eng.policy_actions())
    return step


CLOSED_LOOPS = {      # id -> (scenario, environments, few-cargo)
    '4v8-9x21': ('MATE-4v8-9.yaml', 21, False),              # not a multiple of the four environments of a workgroup
    '4v8-9x21-fewcargo': ('MATE-4v8-9.yaml', 21, True),      # broadcasts
    '8v8-9x9': ('MATE-8v8-9.yaml', 9, False),                # Nc Nc = 64: exactly one round of pairs
    '12v4-2x5': ((12, 4, 2), 5, False),                      # several rounds
    '1v2-2x4': ((1, 2, 2), 4, False),                        # the seat is the only camera: nobody of the team acts
}


@pytest.mark.parametrize('team', ['camera', 'target'])
@pytest.mark.parametrize('case', sorted(CLOSED_LOOPS))
def test_closed_loop_against_seat_ref(case, team, oracle_lib):
    """Random tapes, the seat by TAPE covering 0, a middle slot and n - 1 across the batch, a uniformly random learner, 80 steps (delays are at least 6: second
    sends occur): joint actions within 1e-8 of seat_ref on the oracle environment, masks / goals / bounties / freights exact, seat_obs the seat's row.
    The coverage the case stands for is asserted from seat_ref's own counts (chosen on the CPU: seat_ref.closed_loop without a device gives the same)."""
    from mate_amd.config import read_config
    O = oracle_lib
    scenario, n, few = CLOSED_LOOPS[case]
    cfg = read_config(scenario) if isinstance(scenario, str) else E.scenario(scenario)
    eng, batch = _engine_and_oracle(O, cfg, n, 77, 40, few)
    code = 0 if team == 'camera' else 1
    agents = eng.num_cameras if code == 0 else eng.num_targets
    seats = S.tape_seats(n, agents)
    seat_obs, seat_index, seat_acted = eng.enable_seat(team, torch.from_numpy(seats).to(eng.device))
    device_step = _device_step(eng)
    rows = eng.camera_obs if code == 0 else eng.target_obs
    Nc, Nt = eng.num_cameras, eng.num_targets
    pick = torch.from_numpy(seats.astype(np.int64)).to(eng.device)

    def checked(tape, action, tape_ct, goal_u):
        got = device_step(tape, action, tape_ct, goal_u)
        assert torch.equal(seat_obs, rows[torch.arange(n, device=eng.device), pick])
        assert torch.equal(seat_index.cpu(), torch.from_numpy(seats)) and torch.equal(seat_acted.cpu(), torch.from_numpy(seats))
        return got
    worst, total = S.closed_loop(O, batch, code, seats, 80, 77, step_engine=checked)
    assert worst < 1e-8, worst
    masks = eng.unpack_masks()
    assert np.array_equal(masks['camera_target_view_mask'], batch.gather('camera_target_view_mask').reshape(n, Nc, Nt) != 0)
    sd = eng.state_dict()
    for k in ('tgt_goals', 'bounties', 'freights', 'num_delivered_cargoes'):
        ref = batch.gather(k)
        assert np.array_equal(sd[k].reshape(ref.shape), ref), k
    assert np.abs(sd['tgt_x'] - batch.gather('tgt_x')).max() < 1e-8
    if Nc > 1:
        assert total['sent'] > n * (Nc - 1) * (Nc - 2) and total['told'] >= 1          # second sends, told targets
        assert total['state_to_seat'] == (n * (Nc - 1) if code == 0 else 0)            # every teammate's one 'state' message to the seat
    else:
        assert total['sent'] == 0
    if few:
        assert total['broadcasts'] >= 10                                               # broadcasts (past a target seat)


@pytest.mark.parametrize('team,opposing', [('camera', 'greedy'), ('target', 'greedy'), ('camera', 'heuristic'), ('camera', 'mixture'), ('target', 'mixture')])
def test_twin_engine_bit_for_bit(team, opposing):
    """step_seated on engine A; A's policy_actions() rows of the seat team fed to step_versus_greedy(team, rows) on engine B, same seed: observations,
    scalars, masks and exported state identical over 40 steps with immediate restarts (episodes of 20 steps)."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-4v8-9.yaml', max_episode_steps=20)
    N = 13
    a, b = (Engine(cfg, N, seed=5, first_env_index=3) for _ in range(2))
    other = 'target' if team == 'camera' else 'camera'
    for e in (a, b):
        e.enable_policies()
        if opposing == 'heuristic':
            e.set_target_opponent('heuristic')
        elif opposing == 'mixture':
            e.set_opponent_mixture(other, {'naive': 1.0, 'random': 1.0})
        e.reset()
    a.enable_seat(team, 'draw')
    gen = torch.Generator(device='cpu').manual_seed(8)
    high = torch.tensor([5.0, 5.0] if team == 'camera' else [30.0, 30.0], dtype=torch.float64)      # beyond the action box too
    code = 0 if team == 'camera' else 1
    for s in range(40):
        act = ((torch.rand((N, 2), generator=gen, dtype=torch.float64) * 2 - 1) * high).to(a.device)
        a.step_seated(act, auto_reset=True)
        joint = a.policy_actions()[code]
        assert torch.equal(joint[torch.arange(N, device=a.device), a.seat_acted.long()], act), s
        b.step_versus_greedy(team, joint, auto_reset=True)
        for name in ('camera_obs', 'target_obs', 'scalars', 'masks'):
            assert torch.equal(getattr(a, name), getattr(b, name)), (name, s)
        assert torch.equal(a.export_state(), b.export_state()), s
    assert (a.state_dict()['episode'] >= 2).all()      # (a new engine's first episode is number 0: two restarts)


@pytest.mark.parametrize('auto_reset', [1, 3])
@pytest.mark.parametrize('team', ['camera', 'target'])
def test_seat_across_episodes(team, auto_reset, oracle_lib):
    """DRAW mode, episodes of 12 steps, immediate and batched restarts: seat_acted is the host formula of the episode the step ran in, seat_index that of the
    episode the returned row belongs to (it changes in the call that restarts), seat_obs is that seat's row; an idle environment keeps all three."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    O = oracle_lib
    cfg = read_config('MATE-4v8-9.yaml', max_episode_steps=12)
    N, seed, first = 10, 0x5eed00001234, 900
    eng = Engine(cfg, N, seed=seed, first_env_index=first)
    eng.enable_policies()
    seat_obs, seat_index, seat_acted = eng.enable_seat(team, 'draw')
    eng.reset()
    eng.seat_rows()
    code = 0 if team == 'camera' else 1
    n = eng.num_cameras if code == 0 else eng.num_targets
    rows = eng.camera_obs if code == 0 else eng.target_obs
    formula = lambda episodes: np.array([S.seat_draw(seed, first + e, int(ep), code, n, O.philox) for e, ep in enumerate(episodes)])  # noqa: E731
    before = eng.state_dict()['episode']
    assert np.array_equal(seat_index.cpu().numpy(), formula(before))
    changed = idled = 0
    seen = set()
    act = torch.zeros((N, 2), dtype=torch.float32, device=eng.device)
    for s in range(40):
        kept = (seat_obs.clone(), seat_index.clone(), seat_acted.clone())
        eng.step_seated(act, auto_reset=auto_reset)
        after = eng.state_dict()['episode']
        idle = (eng.scalars[:, 2] == 2).cpu().numpy()
        live = ~idle
        assert np.array_equal(seat_acted.cpu().numpy()[live], formula(before)[live]), s
        assert np.array_equal(seat_index.cpu().numpy()[live], formula(after)[live]), s
        restarted = after != before
        still = torch.from_numpy(idle & ~restarted).to(eng.device)      # idled through the whole call
        for now, then in zip((seat_obs, seat_index, seat_acted), kept):
            assert torch.equal(now[still], then[still]), s
        moved = torch.from_numpy(~(idle & ~restarted)).to(eng.device)
        assert np.array_equal(seat_index.cpu().numpy()[restarted], formula(after)[restarted]), s      # it changes in the call that restarts
        assert torch.equal(seat_obs[moved], rows[torch.arange(N, device=eng.device), seat_index.long()][moved]), s
        changed += int((formula(after) != formula(before)).sum())
        idled += int(still.sum())
        seen |= set(seat_index.cpu().numpy().tolist())
        before = after
    assert (before >= 3).all() and changed >= 3 and len(seen) >= 3
    assert (idled > 0) == (auto_reset > 1)


@pytest.mark.parametrize('team,frame_skip', [('camera', 1), ('target', 1), ('camera', 3)])
def test_graph_replay_equals_the_direct_loop(team, frame_skip):
    """make_stepper(versus='seat', graph_steps=6) against the same calls made directly, bit for bit, restarts inside (episodes of 10 steps); frame_skip = 3 is
    three calls per step with the action held, under the batched restart of interval 3."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-4v8-9.yaml', max_episode_steps=10)
    N = 9
    a, b = (Engine(cfg, N, seed=17) for _ in range(2))
    state = []
    for e in (a, b):
        e.enable_policies()
        e.enable_seat(team, 'draw')
        e.reset()
        act = torch.zeros((N, 2), dtype=torch.float32, device=e.device)
        count = torch.zeros((), dtype=torch.float32, device=e.device)
        state.append((act, count))

    def between_of(act, count):
        def between():
            count.add_(1.0)
            act[:, 0] = torch.sin(count * 0.7 + torch.arange(N, device=act.device)) * 3.0
            act[:, 1] = torch.cos(count * 1.3) * 3.0
        return between
    auto = frame_skip if frame_skip > 1 else 1
    (act_a, count_a), (act_b, count_b) = state
    cam, tgt = (act_a, None) if team == 'camera' else (None, act_a)
    stepper = a.make_stepper(cam, tgt, auto_reset=auto, graph_steps=6, between=between_of(act_a, count_a), versus='seat', frame_skip=frame_skip)
    stepper.run(24)
    torch.cuda.synchronize()
    direct = between_of(act_b, count_b)
    for _ in range(stepper.warmup_steps + 24):
        direct()
        for _ in range(frame_skip):
            b.step_seated(act_b, auto_reset=auto)
    for name in ('camera_obs', 'target_obs', 'scalars', 'masks', 'seat_obs', 'seat_index', 'seat_acted'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    stepper.close()
    assert torch.equal(a.export_state(), b.export_state())
    assert (a.state_dict()['episode'] >= 2).all()      # restarts inside the replayed graphs


def test_enabled_seat_is_inert_and_disable_resets(oracle_lib):
    """An enabled seat with only step_greedy calls gives the flow's bytes without one; after disable_seat() the next step_greedy equals seat_ref with freshly
    reset agents of that team."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    O = oracle_lib
    cfg = read_config('MATE-4v8-9.yaml', max_episode_steps=15)
    a, b = (Engine(cfg, 11, seed=3) for _ in range(2))
    for e in (a, b):
        e.enable_policies()
    a.enable_seat('camera', 1)
    for e in (a, b):
        e.reset()
    for s in range(25):
        for e in (a, b):
            e.step_greedy(auto_reset=True)
        for name in ('camera_obs', 'target_obs', 'scalars', 'masks'):
            assert torch.equal(getattr(a, name), getattr(b, name)), (name, s)
        for x, y in zip(a.policy_actions(), b.policy_actions()):
            assert torch.equal(x, y), s
    # disable: the team's agents start afresh
    n = 6
    eng, batch = _engine_and_oracle(O, read_config('MATE-4v8-9.yaml'), n, 61, 0)
    seats = np.full(n, 2, dtype=np.int32)
    eng.enable_seat('camera', 2)
    device_step = _device_step(eng)
    mirror = [S.SeatAgents(eng.num_cameras, eng.num_targets) for _ in range(n)]
    worst, _ = S.closed_loop(O, batch, 0, seats, 12, 61, step_engine=device_step, agents=mirror)
    assert worst < 1e-8
    eng.disable_seat()
    assert eng.seat_obs is None
    rng = np.random.RandomState(99)
    Nc, Nt = eng.num_cameras, eng.num_targets
    dev = eng.device
    for s in range(8):
        t = {'camera_resample_u': rng.random_sample((n, Nc)), 'camera_sample_u': rng.random_sample((n, Nc, 2)), 'camera_delay': rng.randint(6, 50, size=(n, Nc, Nc)).astype(np.int32),
             'target_choice_u': rng.random_sample((n, Nt)), 'target_resample_u': rng.random_sample((n, Nt)), 'target_sample_u': rng.random_sample((n, Nt, 2)),
             'target_reset_sample_u': rng.random_sample((n, Nt, 2))}
        tape_ct, goal_u = rng.random_sample((n, Nc, Nt)), rng.random_sample((n, Nt))
        eng.step_greedy(policy_tape={k: torch.from_numpy(v).to(dev) for k, v in t.items()}, tape_ct=torch.from_numpy(tape_ct).to(dev),
                        tape_goal=torch.from_numpy(goal_u).to(dev), auto_reset=False)
        cam_act, tgt_act = (x.cpu().numpy() for x in eng.policy_actions())
        for e in range(n):
            agents, env = mirror[e], batch.env(e)
            if s == 0:
                agents.reset_memory(0)
            ca, ta, info = agents.act(S.view_of_oracle(env), t['camera_resample_u'][e], t['camera_sample_u'][e], t['camera_delay'][e], t['target_choice_u'][e],
                                      t['target_resample_u'][e], t['target_sample_u'][e], t['target_reset_sample_u'][e])
            assert np.abs(ca - cam_act[e]).max() < 1e-8 and np.abs(ta - tgt_act[e]).max() < 1e-8, (s, e)
            if s == 0:
                assert info['sent'].sum() == Nc * (Nc - 1)                             # all four cameras say 'state' again: a fresh team
            env.step(ca, ta, tape_ct[e], goal_u[e])


def test_refusals_leave_the_engine_usable():
    """Every refusal of include/mate_engine.h's seat block, each leaving the engine as it was and usable."""
    import ctypes
    from mate_amd._native import EngineError
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    EINVAL, ESTATE = -1, -4
    cfg = read_config('MATE-4v8-9.yaml', shuffle_entities=False)
    N = 6
    eng = Engine(cfg, N, seed=1)
    Nt = eng.num_targets

    def refused(code, call, *args, **kw):
        with pytest.raises(EngineError) as err:
            call(*args, **kw)
        assert err.value.code == code, err.value

    def raw_enable(team, mode, fixed, tape, obs, index, acted):
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        return eng.lib.mate_engine_enable_seat(eng._h, team, mode, fixed, p(tape), p(obs), p(index), p(acted))
    refused(ESTATE, eng.enable_seat, 'camera')                                         # before policy_enable
    assert eng.seat_obs is None
    eng.enable_policies()
    eng.reset()
    refused(EINVAL, eng.enable_seat, 'camera', 4)                                      # a fixed seat outside [0, n)
    obs = torch.zeros(N * eng.camera_obs_dim + 4, dtype=torch.float32, device=eng.device)
    index, acted = (torch.zeros(N, dtype=torch.int32, device=eng.device) for _ in range(2))
    assert raw_enable(0, 0, 0, None, obs[1:], index, acted) == EINVAL                  # a misaligned buffer
    assert raw_enable(2, 0, 0, None, obs, index, acted) == EINVAL                      # a team that is neither
    assert raw_enable(0, 3, 0, None, obs, index, acted) == EINVAL                      # no such mode
    assert raw_enable(0, 2, 0, None, obs, index, acted) == EINVAL                      # TAPE without a tape
    assert raw_enable(0, 0, 0, None, obs, None, acted) == EINVAL                       # a missing buffer
    nocam = Engine(E.scenario((0, 5, 64)), 2, seed=1)
    nocam.enable_policies()
    refused(EINVAL, nocam.enable_seat, 'camera')                                       # a team without agents
    nocam.close()
    # a seat team with a Heuristic selection, a mixture other than {Greedy}, a channel set; the opposing team's live channel
    eng.set_target_opponent('heuristic')
    refused(ESTATE, eng.enable_seat, 'target')
    eng.set_target_opponent('greedy')
    eng.set_opponent_mixture('camera', {'greedy': 1.0, 'naive': 1.0})
    refused(ESTATE, eng.enable_seat, 'camera')
    eng.clear_opponent_mixture('camera')
    eng.set_opponent_mixture('camera', {'greedy': 1.0})                                # ({Greedy} alone is the plain agents)
    eng.enable_seat('camera')
    eng.disable_seat()
    eng.clear_opponent_mixture('camera')
    eng.set_channel('camera', dropout_rate=0.5)
    refused(ESTATE, eng.enable_seat, 'camera')
    refused(ESTATE, eng.enable_seat, 'target')
    eng.clear_channel('camera')
    assert eng.seat_obs is None
    assert eng.lib.mate_engine_step_seated(eng._h, None, None, 1, None) == ESTATE      # no seat
    # ... and installing any of them on the seat team while the seat is enabled
    eng.enable_seat('target')
    refused(ESTATE, eng.enable_seat, 'camera')                                         # one seat team per engine
    assert eng.seat_team == 1
    refused(ESTATE, eng.set_target_opponent, 'heuristic')
    refused(ESTATE, eng.set_opponent_mixture, 'target', {'naive': 1.0})
    refused(ESTATE, eng.set_channel, 'target', disabled=True)
    assert eng.target_agent == 'greedy' and eng.mixtures[1] is None and eng.channels[1] is None
    act = torch.zeros((N, 2), dtype=torch.float64, device=eng.device)
    eng.set_channel('camera', disabled=True)                                           # the opposing team's channel goes live afterwards: the call is refused
    refused(ESTATE, eng.step_seated, act)
    eng.clear_channel('camera')
    refused(EINVAL, eng.step_seated, None)                                             # no action
    eng.set_camera_opponent('heuristic')                                               # the opposing team may be anything
    eng.step_seated(act)
    eng.set_camera_opponent('greedy')
    eng.step_seated(act)
    assert (eng.seat_index == Nt - 1).all() and (eng.seat_acted == Nt - 1).all()       # 'auto' with shuffle_entities off
    assert torch.equal(eng.seat_obs, eng.target_obs[:, Nt - 1])
    eng.rollout_greedy(4)                                                              # the fused flows are untouched
    eng.disable_seat()
    eng.step_greedy()


def test_environment_and_evaluation_script():
    """BatchedMultiAgentTracking(single_agent=...): reset() returns the seat's rows, step_single the wrapper's four values with info['seat']; the evaluation
    script's --single-agent runs a random learner in the seat and reports episode records as ever (in this process: no child is started)."""
    from mate_amd import evaluate
    from mate_amd.environment import BatchedMultiAgentTracking
    N = 6
    env = BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=N, seed=2, single_agent='camera', target_agent='heuristic', max_episode_steps=8)
    eng = env.engine
    every = torch.arange(N, device=eng.device)
    obs = env.reset()
    assert obs is eng.seat_obs and obs.shape == (N, eng.camera_obs_dim) and torch.equal(obs, eng.camera_obs[every, eng.seat_index.long()])
    assert eng.seat_mode == ('draw' if env.config['shuffle_entities'] else 'fixed') and eng.target_agent == 'heuristic'
    act = torch.zeros((N, 2), dtype=torch.float32, device=eng.device)
    finished = 0
    for s in range(20):
        obs, reward, done, info = env.step_single(act)
        assert obs.shape == (N, eng.camera_obs_dim) and reward.shape == (N,) and done.shape == (N,) and done.dtype == torch.bool
        assert info['seat'] is eng.seat_index and info['seat_acted'] is eng.seat_acted and 'coverage_rate' in info
        assert torch.equal(reward, eng.scalars[:, 0]) and torch.equal(obs, eng.camera_obs[every, info['seat'].long()])
        finished += int(done.sum())
    assert finished >= 2 * N
    env.close()
    records = evaluate.main(['--config', 'MATE-4v8-9.yaml', '--num-envs', '8', '--single-agent', 'target', '--episodes', '8', '--max-episode-steps', '10', '--seed', '4'])
    assert records.shape == (8, 16) and np.isfinite(records[:, :4]).all()
