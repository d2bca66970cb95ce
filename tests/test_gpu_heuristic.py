"""GPU parity of the Heuristic target opponent (mate_engine_set_target_opponent, csrc/opponent_rows.hpp): HeuristicTargetAgent
(mate/agents/heuristic.py:290-337) on the device, closed loop against the reference's recording (fixtures heuristic_*.npz of
tests/golden/make_heuristic_golden.py) and, on Philox draws, against the NumPy restatement of tests/heuristic_ref.py that
tests/test_heuristic_host.py pins to the same recording."""
import numpy as np
import pytest
import torch

import golden_util as G
import gpu_util as U
from heuristic_ref import heuristic_drift

pytestmark = pytest.mark.gpu

FIXTURES = ['heuristic_4v8-9_s51', 'heuristic_8v8-9_s52', 'heuristic_4v2-9_s53']
ESTATE, EINVAL = -4, -1
ONE_LAUNCH_FLOWS = (3, 4)      # FLOW_GREEDY / FLOW_STEP_GREEDY (csrc/engine_kernels.hpp): the agents and the step in one kernel


def _replay(name, versus_camera):
    """The reference's episode replayed with recorded agent and environment draws, N = 2, f64 observations: exactly
    test_greedy_policies_closed_loop's loop with the heuristic opponent on (step_greedy, or the MultiCamera form with the recorded camera actions)."""
    fx = G.load(name + '.npz')
    N = 2
    eng = U.engine_from_fixture(fx, N, obs_dtype=torch.float64)
    eng.enable_policies(target_agent='heuristic')
    Nc = eng.num_cameras
    dev = eng.device
    tape0 = torch.from_numpy(np.where(fx['reset/camera_target_view_mask'], 1.0, 0.0)[None].repeat(N, 0)).to(dev)
    eng.observe(tape_ct=tape0)
    m0 = eng.unpack_masks()
    assert np.array_equal(m0['camera_target_view_mask'][0], fx['reset/camera_target_view_mask'])
    assert np.array_equal(m0['target_camera_view_mask'][1], fx['reset/target_camera_view_mask'])

    def bc(a, dtype=np.float64):
        a = np.asarray(a)
        return torch.from_numpy(np.broadcast_to(a, (N,) + a.shape).astype(dtype).copy()).to(dev)

    T = len(fx['step/done'])
    worst = {'greedy': 0.0, 'final': 0.0, 'camera': 0.0, 'xy': 0.0}
    for s in range(T):
        tape = {
            'camera_resample_u': bc(np.nan_to_num(fx['step/agent_cam_binom_u'][s], nan=0.0)),
            'camera_sample_u': bc(np.nan_to_num(fx['step/agent_cam_sample_u'][s], nan=0.0)),
            'camera_delay': bc(fx['step/agent_cam_delay'][s], np.int32),
            'target_choice_u': bc(np.nan_to_num(fx['step/agent_tgt_choice_u'][s], nan=0.0)),
            'target_resample_u': bc(np.nan_to_num(fx['step/agent_tgt_binom_u'][s], nan=0.0)),
            'target_sample_u': bc(np.nan_to_num(fx['step/agent_tgt_sample_u'][s], nan=0.0)),
            'target_reset_sample_u': bc(fx['agent/tgt_reset_sample_u']),
        }
        env_tape = bc(np.nan_to_num(fx['step/tape_ct'][s], nan=0.0))
        goal_tape = bc(np.nan_to_num(fx['step/goal_u'][s], nan=0.0))
        if versus_camera:
            eng.step_versus_greedy('camera', bc(fx['step/cam_act'][s]), policy_tape=tape, tape_ct=env_tape, tape_goal=goal_tape, auto_reset=False)
        else:
            eng.step_greedy(policy_tape=tape, tape_ct=env_tape, tape_goal=goal_tape, auto_reset=False)
        assert eng.last_flow not in ONE_LAUNCH_FLOWS
        cam_act, tgt_act, greedy = (a.cpu().numpy() for a in eng.policy_actions(greedy_targets=True))
        sd = eng.state_dict()
        for e in range(N):
            worst['greedy'] = max(worst['greedy'], np.abs(greedy[e] - fx['step/tgt_act_greedy'][s]).max())
            worst['final'] = max(worst['final'], np.abs(tgt_act[e] - fx['step/tgt_act'][s]).max())
            if not versus_camera:
                worst['camera'] = max(worst['camera'], np.abs(cam_act[e] - fx['step/cam_act'][s]).max())
            worst['xy'] = max(worst['xy'], np.abs(sd['tgt_x'][e] - fx['step/tgt_xy'][s][:, 0]).max(), np.abs(sd['tgt_y'][e] - fx['step/tgt_xy'][s][:, 1]).max())
        assert worst['greedy'] < 1e-8 and worst['final'] < 1e-8 and worst['camera'] < 1e-8 and worst['xy'] < 1e-8, (s, worst)
        masks = eng.unpack_masks()
        assert np.array_equal(masks['camera_target_view_mask'][0], fx['step/camera_target_view_mask'][s]), s
        assert np.array_equal(sd['tgt_goals'][0], fx['step/tgt_goals'][s].astype(np.float64)), s
        assert np.array_equal(sd['bounties'][1], fx['step/bounties'][s].astype(np.float64)), s
        assert sd['episode_reward'][0] == fx['step/episode_reward'][s], s
    print(name, 'versus camera' if versus_camera else 'step_greedy', T, 'steps, worst differences', worst)
    assert np.abs(fx['step/tgt_act'] - fx['step/tgt_act_greedy']).max() > 1.0      # (the drift is in the recording)


@pytest.mark.parametrize('name', FIXTURES)
def test_heuristic_targets_closed_loop(name):
    _replay(name, versus_camera=False)


@pytest.mark.parametrize('name', FIXTURES)
def test_multi_camera_versus_heuristic_targets_closed_loop(name):
    _replay(name, versus_camera=True)


def _restatement_inputs(eng, cfg):
    """What the agents of the NEXT step act on, from the engine: the state and the engine's mask words as the last call left them."""
    sd = eng.state_dict()
    cam = U.scenario_tables(cfg)['camera']
    theta_min, rmax = cam['min_viewing_angle'], cam['max_sight_range']
    sensed = eng.unpack_masks()['target_camera_view_mask']
    with np.errstate(divide='ignore'):
        sight = np.sqrt(theta_min * rmax * rmax / sd['cam_theta'])
    return dict(tgt_xy=np.stack([sd['tgt_x'], sd['tgt_y']], axis=-1), step_size=cfg['target']['step_size'] / sd['tgt_capacity'],
                cam_xy=np.stack([sd['cam_x'], sd['cam_y']], axis=-1), cam_phi=sd['cam_phi'], cam_theta=sd['cam_theta'], cam_sight=sight, sensed=sensed)


@pytest.mark.parametrize('config,n,steps,kw,flow', [
    ('MATE-4v8-9.yaml', 96, 150, {'max_episode_steps': 60}, 'versus'),      # immediate restarts fall inside the run
    ('MATE-4v8-9.yaml', 96, 150, {'max_episode_steps': 60}, 'selected'),
    ('MATE-8v8-9.yaml', 65, 40, {}, 'versus'),                              # a partial tile: 16 environments per workgroup plus one
    ('MATE-2v4-0.yaml', 33, 60, {}, 'versus'),                              # no obstacles, sub-wave shape
    ('MATE-Navigation.yaml', 17, 40, {}, 'greedy'),                         # no cameras: a plain copy
    # tests/shape_edges.py ATTACHED_CASES (n, seed and first_env_index are the case's): target rows of NJ = 15 and 12 bits and
    # camera_target_view_mask rows that cross 32-bit words; sixteen cameras: cam_xy[..][32] full, the field mask (1u << 16) - 1u, NJ = 34
    # and 41; no cameras on the generic kernels
    ('7v5-3', None, 40, {}, 'versus'),
    ('5v7-0', None, 40, {}, 'versus'),
    ('16v15-3', None, 40, {}, 'selected'),
    ('16v16-9', None, 40, {}, 'versus'),
    ('0v5-64', None, 40, {}, 'greedy'),
])
def test_heuristic_batch_against_the_restatement(config, n, steps, kw, flow):
    """On Philox draws: the state and the masks are read before every step, the Greedy and the final target actions after it;
    final must equal restatement(Greedy) to 1e-9 wherever no branch condition lies within 1e-9 (relative) of equality."""
    import shape_edges
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    shipped = config.endswith('.yaml')
    if shipped:
        cfg, seeds = read_config(config, **kw), dict(seed=23)
    else:
        case = shape_edges.attached_case(config)
        cfg, n, seeds = shape_edges.case_scenario(case), case.n, dict(seed=case.seed, first_env_index=case.first)
    eng = Engine(cfg, n, **seeds)
    assert shipped or not eng.specialised
    eng.enable_policies(target_agent='heuristic')
    eng.reset()
    Nc, Nt = eng.num_cameras, eng.num_targets
    twin = None
    if Nc == 0:      # the whole run against an engine left on Greedy
        twin = Engine(cfg, n, **seeds)
        twin.enable_policies()
        twin.reset()
    straddling = {c: 0 for c in shape_edges.straddling_rows(Nc, Nt)}
    gen = torch.Generator(device='cpu').manual_seed(5)
    mine = torch.zeros((n, max(Nc, 1), 2), device=eng.device)
    if flow == 'selected':
        selection = eng.enable_selection(multi_selection=True)
    entries = skipped = drifted = rejected = 0
    worst = 0.0
    restarts = 0
    for s in range(steps):
        before = _restatement_inputs(eng, cfg)
        for c, frames in shape_edges.straddling_frames(eng.unpack_masks()['camera_target_view_mask']).items():      # (the selection executor's view)
            straddling[c] += frames
        episode_before = eng.state_dict()['episode'].copy()
        if flow == 'versus':
            mine.copy_((torch.rand(mine.shape, generator=gen) * 2.0 - 1.0) * 5.0)
            eng.step_versus_greedy('camera', mine, auto_reset=True)
        elif flow == 'selected':
            selection.copy_(torch.randint(0, 1 << Nt, selection.shape, generator=gen, dtype=torch.int32))
            eng.step_selected(auto_reset=True)
        else:
            eng.step_greedy(auto_reset=True)
        assert eng.last_flow not in ONE_LAUNCH_FLOWS
        _, final, greedy = (a.cpu().numpy() for a in eng.policy_actions(greedy_targets=True))
        restarts += int((eng.state_dict()['episode'] != episode_before).sum())
        if twin is not None:
            twin.step_greedy(auto_reset=True)
            assert np.array_equal(final, greedy), s
            for a, b in ((eng.scalars, twin.scalars), (eng.target_obs, twin.target_obs), (eng.masks, twin.masks), (eng.export_state(), twin.export_state())):
                assert torch.equal(a, b), s
            continue
        expect, info = heuristic_drift(greedy, noise_scale=0.5, **before)
        near = info['margin'] <= 1e-9
        entries += near.size
        skipped += int(near.sum())
        drifted += int(info['drifted'].sum())
        rejected += int(info['rejected'].sum())
        worst = max(worst, float(np.abs(final - expect)[~near].max()))
        assert worst < 1e-9, (s, worst)
        assert np.array_equal(final[~info['drifted'] & ~near], greedy[~info['drifted'] & ~near]), s      # unchanged means the same bits
    if twin is not None:
        return
    print(config, n, flow, 'entries', entries, 'skipped', skipped, 'drifted', drifted / entries, 'rejected', rejected / entries, 'worst', worst, 'restarts', restarts)
    assert skipped <= 0.001 * entries, (skipped, entries)
    if shipped:
        assert drifted >= 0.05 * entries and rejected >= 0.01 * entries, (drifted, rejected, entries)
    else:      # (those floors were set on the shipped scenarios: here both branches must occur)
        assert drifted > 0 and rejected > 0, (drifted, rejected, entries)
        if straddling:
            print(config, flow, 'frames per straddling camera_target_view_mask row', straddling)
            assert min(straddling.values()) >= 1, straddling
    if 'max_episode_steps' in kw:
        assert restarts >= 2 * n      # every environment restarted inside the run, twice


def test_batched_restarts_and_graph_replay():
    """auto_reset = 4 over episodes of 25 steps: an environment that idles (done = 2) until the interval's restart keeps its Greedy row;
    the graph stepper's replay of whole intervals equals the direct calls bit for bit."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-4v8-9.yaml', max_episode_steps=25)
    n, k = 64, 4
    direct, graphed = Engine(cfg, n, seed=9), Engine(cfg, n, seed=9)
    for eng in (direct, graphed):
        eng.enable_policies(target_agent='heuristic')
        eng.reset()
    mine = [torch.zeros((n, eng.num_cameras, 2), device=eng.device) for eng in (direct, graphed)]
    counters = [torch.zeros((), device=direct.device) for _ in range(2)]

    def policy(i):
        def between():
            counters[i].add_(1.0)
            mine[i].copy_((torch.sin(counters[i]) * 4.0).expand_as(mine[i]))
        return between

    stepper = graphed.make_stepper(mine[1], None, auto_reset=k, graph_steps=2 * k, between=policy(1), versus='camera')
    assert stepper.graph is not None
    total = stepper.warmup_steps + 5 * 2 * k      # ten restart intervals behind the warm-up one: episodes end at step 25
    idle_rows = moved_rows = 0
    for s in range(total):
        policy(0)()
        direct.step_versus_greedy('camera', mine[0], auto_reset=k)
        _, final, greedy = direct.policy_actions(greedy_targets=True)
        idle = direct.scalars[:, 2] == 2
        assert torch.equal(final[idle], greedy[idle]), s
        idle_rows += int(idle.sum())
        moved_rows += int((final[~idle] != greedy[~idle]).any(-1).any(-1).sum())
    assert idle_rows > 0 and moved_rows > 0
    for _ in range(5):
        stepper.run(2 * k)
    for a, b in ((direct.scalars, graphed.scalars), (direct.masks, graphed.masks), (direct.camera_obs, graphed.camera_obs), (direct.target_obs, graphed.target_obs),
                 (direct.export_state(), graphed.export_state())):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for a, b in zip(direct.policy_actions(greedy_targets=True), graphed.policy_actions(greedy_targets=True)):
        assert torch.equal(a, b)
    stepper.close()
    assert (direct.state_dict()['episode'] >= 2).all()


def test_greedy_is_untouched_by_the_switch():
    """An engine that switched to Heuristic and back -- before the first step and again in the middle -- is bit-identical to one that never did,
    and runs the one-launch form again."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-4v8-9.yaml', max_episode_steps=30)
    n = 96
    plain, switched = Engine(cfg, n, seed=3), Engine(cfg, n, seed=3)
    for eng in (plain, switched):
        eng.enable_policies()
        eng.reset()
    switched.set_target_opponent('heuristic')
    switched.set_target_opponent('greedy')
    gen = torch.Generator(device='cpu').manual_seed(1)
    mine = torch.zeros((n, plain.num_cameras, 2), device=plain.device)
    for s in range(50):
        mine.copy_((torch.rand(mine.shape, generator=gen) * 2.0 - 1.0) * 5.0)
        if s == 25:
            switched.set_target_opponent('heuristic')
            assert switched.target_agent == 'heuristic'
            switched.set_target_opponent('greedy')
        for eng in (plain, switched):
            eng.step_versus_greedy('camera', mine, auto_reset=True)
        assert switched.last_flow == plain.last_flow and plain.last_flow in ONE_LAUNCH_FLOWS, s
        for a, b in ((plain.scalars, switched.scalars), (plain.masks, switched.masks), (plain.camera_obs, switched.camera_obs), (plain.target_obs, switched.target_obs)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), s
        _, final, greedy = switched.policy_actions(greedy_targets=True)
        assert torch.equal(final, greedy) and torch.equal(final, plain.policy_actions()[1])
    assert torch.equal(plain.export_state(), switched.export_state())


def test_refusals_name_the_opponent_and_leave_the_engine_usable():
    from mate_amd._native import EngineError
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-4v8-9.yaml')
    n = 32
    eng = Engine(cfg, n, seed=2)
    with pytest.raises(EngineError, match='policy_enable') as err:
        eng.set_target_opponent('heuristic')
    assert err.value.code == ESTATE and eng.target_agent == 'greedy'
    with pytest.raises(ValueError, match='target_agent'):
        eng.set_target_opponent('smart')
    eng.enable_policies(target_agent='heuristic')
    eng.reset()
    mine = torch.zeros((n, eng.num_cameras, 2), device=eng.device)
    before = eng.export_state().clone()
    with pytest.raises(EngineError, match='heuristic') as err:
        eng.rollout_greedy(4)
    assert err.value.code == ESTATE
    with pytest.raises(EngineError, match='heuristic') as err:
        eng.rollout_versus_greedy('camera', mine, 4)
    assert err.value.code == ESTATE
    for mode in ('enhanced', 'shared'):
        with pytest.raises(EngineError, match='heuristic') as err:
            eng.set_obs_mode(target=mode)
        assert err.value.code == EINVAL
    with pytest.raises(ValueError, match='heuristic'):
        eng.make_stepper(mine, None, versus='camera', frame_skip=4)
    with pytest.raises(ValueError, match='heuristic'):
        eng.make_stepper(mine, None, versus='camera', frame_skip=4, graph_steps=2)
    assert torch.equal(before, eng.export_state())      # nothing ran
    # the caller plays the targets: unaffected, the fused launch included; and the engine steps on
    theirs = torch.zeros((n, eng.num_targets, 2), device=eng.device)
    eng.rollout_versus_greedy('target', theirs, 3)
    eng.step_versus_greedy('target', theirs)
    assert eng.last_flow in ONE_LAUNCH_FLOWS
    moved = False
    for _ in range(30):      # (right behind a reset few targets sense a camera: the drift shows within some steps)
        eng.step_versus_greedy('camera', mine)
        assert eng.last_flow not in ONE_LAUNCH_FLOWS
        _, final, greedy = eng.policy_actions(greedy_targets=True)
        moved = moved or not torch.equal(final, greedy)
    assert moved
    # ... and the other way round: Heuristic is refused under a non-plain target team mode
    eng.set_target_opponent('greedy')
    eng.set_obs_mode(target='enhanced')
    with pytest.raises(EngineError, match='plain rows') as err:
        eng.set_target_opponent('heuristic')
    assert err.value.code == EINVAL and eng.target_agent == 'greedy'
    eng.set_obs_mode(camera='shared')
    eng.set_target_opponent('heuristic')
    eng.step_greedy()
    # policy_actions is what the LAST step consumed: behind a call in which the caller played the targets, not the drift launch's buffer
    eng.set_obs_mode()
    ones = torch.ones((n, eng.num_targets, 2), device=eng.device)
    eng.step_versus_greedy('target', ones)
    assert eng.last_flow in ONE_LAUNCH_FLOWS
    assert torch.equal(eng.policy_actions()[1], ones.double())


def test_environment_classes_take_the_target_agent():
    import mate_amd
    env = mate_amd.BatchedMultiAgentTracking('MATE-4v2-9.yaml', num_envs=8, target_agent='heuristic')
    env.reset()
    assert env.engine.target_agent == 'heuristic'
    env.step_versus_greedy('camera', torch.zeros((8, env.num_cameras, 2), device=env.device))
    assert env.engine.last_flow not in ONE_LAUNCH_FLOWS
    single = mate_amd.MultiAgentTracking('MATE-4v2-9.yaml')
    single.enable_greedy_policies(target_agent='heuristic')
    single.seed(0)
    single.reset()
    single.step_greedy()
    assert single.engine.target_agent == 'heuristic'
