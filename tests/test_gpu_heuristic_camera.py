"""GPU parity of the Heuristic camera opponent (mate_engine_set_camera_opponent, csrc/opponent_rows.hpp): HeuristicCameraAgent
(mate/agents/heuristic.py:17-287) on the device, closed loop against the reference's recording (fixtures heuristic_camera_*.npz of
tests/golden/make_heuristic_camera_golden.py) and, on Philox draws, against the NumPy restatement of tests/heuristic_camera_ref.py that
tests/test_heuristic_camera_host.py pins to the same recording."""
import numpy as np
import pytest
import torch

import golden_util as G
import gpu_util as U
from heuristic_camera_ref import heuristic_cameras

pytestmark = pytest.mark.gpu

FIXTURES = ['heuristic_camera_4v8-9_s61', 'heuristic_camera_8v8-9_s62', 'heuristic_camera_2v4-0_s65']
ESTATE, EINVAL = -4, -1
ONE_LAUNCH_FLOWS = (3, 4)      # FLOW_GREEDY / FLOW_STEP_GREEDY (csrc/engine_kernels.hpp): the agents and the step in one kernel


def _tables(cfg):
    from mate_amd.heuristic_tables import heuristic_camera_tables
    cam = U.scenario_tables(cfg)['camera']
    return heuristic_camera_tables(cam['max_sight_range'], cam['min_viewing_angle'])


def _replay(name, versus_target):
    """The reference's episode replayed with recorded agent and environment draws, N = 2, f64 observations: step_greedy, or the MultiTarget
    form with the recorded target actions."""
    fx = G.load(name + '.npz')
    N = 2
    eng = U.engine_from_fixture(fx, N, obs_dtype=torch.float64)
    eng.enable_policies(camera_agent='heuristic')
    Nc = eng.num_cameras
    dev = eng.device
    tape0 = torch.from_numpy(np.where(fx['reset/camera_target_view_mask'], 1.0, 0.0)[None].repeat(N, 0)).to(dev)
    eng.observe(tape_ct=tape0)
    m0 = eng.unpack_masks()
    assert np.array_equal(m0['camera_target_view_mask'][0], fx['reset/camera_target_view_mask'])

    def bc(a, dtype=np.float64):
        a = np.asarray(a)
        return torch.from_numpy(np.broadcast_to(a, (N,) + a.shape).astype(dtype).copy()).to(dev)

    perms = torch.zeros((N, 32, Nc), dtype=torch.int8, device=dev)
    used = torch.full((N, 32, Nc), -1, dtype=torch.int8, device=dev)
    eng.heuristic_camera_tape(permutations=perms, record=used)
    T = len(fx['step/done'])
    worst = {'camera': 0.0, 'target': 0.0, 'xy': 0.0, 'pose': 0.0}
    for s in range(T):
        tape = {
            'camera_resample_u': bc(np.nan_to_num(fx['step/agent_cam_binom_u'][s], nan=0.0)),
            'camera_sample_u': bc(np.nan_to_num(fx['step/agent_cam_sample_u'][s], nan=0.0)),
            'target_choice_u': bc(np.nan_to_num(fx['step/agent_tgt_choice_u'][s], nan=0.0)),
            'target_resample_u': bc(np.nan_to_num(fx['step/agent_tgt_binom_u'][s], nan=0.0)),
            'target_sample_u': bc(np.nan_to_num(fx['step/agent_tgt_sample_u'][s], nan=0.0)),
            'target_reset_sample_u': bc(fx['agent/tgt_reset_sample_u']),
        }
        perms.copy_(bc(fx['step/hcam_permutations'][s], np.int8))
        env_tape = bc(np.nan_to_num(fx['step/tape_ct'][s], nan=0.0))
        goal_tape = bc(np.nan_to_num(fx['step/goal_u'][s], nan=0.0))
        if versus_target:
            eng.step_versus_greedy('target', bc(fx['step/tgt_act'][s]), policy_tape=tape, tape_ct=env_tape, tape_goal=goal_tape, auto_reset=False)
        else:
            eng.step_greedy(policy_tape=tape, tape_ct=env_tape, tape_goal=goal_tape, auto_reset=False)
        assert eng.last_flow not in ONE_LAUNCH_FLOWS
        cam_act, tgt_act = (a.cpu().numpy() for a in eng.policy_actions())
        goals, index = (a.cpu().numpy() for a in eng.heuristic_camera_goals())
        assert torch.equal(used, perms), s
        sd = eng.state_dict()
        for e in range(N):
            assert np.array_equal(index[e], fx['step/hcam_goal_index'][s]), (s, e, index[e], fx['step/hcam_goal_index'][s])
            assert np.array_equal(np.nan_to_num(goals[e], nan=1e9), np.nan_to_num(fx['step/hcam_goal'][s], nan=1e9)), (s, e)
            worst['camera'] = max(worst['camera'], np.abs(cam_act[e] - fx['step/cam_act'][s]).max())
            if not versus_target:
                worst['target'] = max(worst['target'], np.abs(tgt_act[e] - fx['step/tgt_act'][s]).max())
            worst['xy'] = max(worst['xy'], np.abs(sd['tgt_x'][e] - fx['step/tgt_xy'][s][:, 0]).max(), np.abs(sd['tgt_y'][e] - fx['step/tgt_xy'][s][:, 1]).max())
            worst['pose'] = max(worst['pose'], np.abs(sd['cam_phi'][e] - fx['step/cam_phi'][s]).max(), np.abs(sd['cam_theta'][e] - fx['step/cam_theta'][s]).max())
        assert max(worst.values()) < 1e-8, (s, worst)
        masks = eng.unpack_masks()
        assert np.array_equal(masks['camera_target_view_mask'][0], fx['step/camera_target_view_mask'][s]), s
        assert np.array_equal(sd['tgt_goals'][0], fx['step/tgt_goals'][s].astype(np.float64)), s
        assert np.array_equal(sd['bounties'][1], fx['step/bounties'][s].astype(np.float64)), s
        assert sd['episode_reward'][0] == fx['step/episode_reward'][s], s
    print(name, 'versus target' if versus_target else 'step_greedy', T, 'steps, worst differences', worst)
    assert (fx['step/hcam_goal_index'] >= 0).any() and (fx['step/hcam_goal_index'] < 0).any()


@pytest.mark.parametrize('name', FIXTURES)
def test_heuristic_cameras_closed_loop(name):
    _replay(name, versus_target=False)


@pytest.mark.parametrize('name', FIXTURES)
def test_multi_target_versus_heuristic_cameras_closed_loop(name):
    _replay(name, versus_target=True)


@pytest.mark.parametrize('config,n,steps,kw', [
    ('MATE-4v8-9.yaml', 33, 30, {'max_episode_steps': 12}),      # restarts fall inside the run
    ('MATE-8v8-9.yaml', 17, 20, {}),
    ('MATE-2v4-0.yaml', 33, 30, {}),
    # tests/shape_edges.py ATTACHED_CASES (n, seed and first_env_index are the case's): camera_target_view_mask rows that cross 32-bit
    # words; sixteen by sixteen -- 121 KB of accumulators, sixteen-bit masks, fifteen Fisher-Yates draws
    ('7v5-3', None, 12, {}),
    ('16v16-9', None, 12, {}),
])
def test_heuristic_cameras_batch_against_the_restatement(config, n, steps, kw):
    """On Philox draws: the state and the masks are read before every step, the permutations (record_dev), the goals and the camera
    actions after it.  Goal indices must equal the restatement's wherever its decision margin exceeds 1e-9 (at most 0.1 % of the
    camera-steps excused, the share test_gpu_heuristic.py allows), the actions of cameras with a goal agree to 1e-9 there, and a
    no-goal action is bitwise the previous one or lies inside the action box.

    Which margin excuses: only the in-range test's, the one decision whose arithmetic differs between the two sides (the device's norm2
    fuses its multiply-add).  The nearest grid point, the picks and the winner are specified operation by operation -- f64 products, sums
    in list order, true divisions, correctly rounded roots, table entries that are the same bytes -- so the device must reproduce them bit
    for bit, and it is held to that: on these scenarios one environment-step in a hundred has two pick values a unit in the last place
    apart (sums of mirror-symmetric table rows added in another order: observed 1.2e-16 relative on MATE-8v8-9, MATE-2v4-0 and 7v5-3), far
    more than the 0.1 % that may be excused, and every one of them must come out as the restatement's.  Those near-ties are printed and
    counted (`near`).  This asks more than `margin > 1e-9` would: the environments compared are a superset."""
    import shape_edges
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    shipped = config.endswith('.yaml')
    if shipped:
        cfg, seeds = read_config(config, **kw), dict(seed=29)
    else:
        case = shape_edges.attached_case(config)
        cfg, n, seeds = shape_edges.case_scenario(case), case.n, dict(seed=case.seed, first_env_index=case.first)
    eng = Engine(cfg, n, **seeds)
    eng.enable_policies(camera_agent='heuristic')
    eng.reset()
    Nc, Nt = eng.num_cameras, eng.num_targets
    cam = U.scenario_tables(cfg)['camera']
    rot, zoom, rmax = cam['rotation_step'], cam['zooming_step'], cam['max_sight_range']
    tables = _tables(cfg)
    used = torch.full((n, 32, Nc), -1, dtype=torch.int8, device=eng.device)
    eng.heuristic_camera_tape(record=used)
    gen = torch.Generator(device='cpu').manual_seed(7)
    theirs = torch.zeros((n, Nt, 2), device=eng.device)
    prev = np.zeros((n, Nc, 2))
    last_episode = np.full(n, -1)
    camera_steps = excused = with_goal = kept = resampled = restarts = near = 0
    worst = 0.0
    for s in range(steps):
        sd = eng.state_dict()
        seen = eng.unpack_masks()['camera_target_view_mask']
        prev[sd['episode'] != last_episode] = 0.0      # the agents' reset at the team's first acting call of an episode
        restarts += int((sd['episode'] != last_episode).sum())
        last_episode = sd['episode'].copy()
        theirs.copy_((torch.rand(theirs.shape, generator=gen) * 2.0 - 1.0) * 20.0)
        eng.step_versus_greedy('target', theirs, auto_reset=True)
        assert eng.last_flow not in ONE_LAUNCH_FLOWS
        action = eng.policy_actions()[0].cpu().numpy()
        goals, index = (a.cpu().numpy() for a in eng.heuristic_camera_goals())
        perms = used.cpu().numpy()
        assert (np.sort(perms, axis=-1) == np.arange(Nc, dtype=np.int8)).all(), s      # every recorded row is a permutation
        expect, want_index, want_goal, info = heuristic_cameras(
            cam_xy=np.stack([sd['cam_x'], sd['cam_y']], axis=-1), cam_phi=sd['cam_phi'], cam_theta=sd['cam_theta'],
            tgt_xy=np.stack([sd['tgt_x'], sd['tgt_y']], axis=-1), seen=seen, permutations=perms, prev_action=prev,
            binom_u=np.zeros((n, Nc)), sample_u=np.zeros((n, Nc, 2)), rot=rot, zoom=zoom, rmax=rmax, tables=tables)
        sure = info['margins']['range'] > 1e-9                                         # [n]
        for b in np.flatnonzero(~(info['margin'] > 1e-9)):
            near += 1
            print(config, 'step', s, 'environment', b, 'margins', {key: float(value[b]) for key, value in info['margins'].items()})
        camera_steps += n * Nc
        excused += int((~sure).sum()) * Nc
        assert np.array_equal(index[sure], want_index[sure]), (s, np.argwhere(index != want_index)[:5])
        has = (want_index >= 0) & sure[:, None]
        with_goal += int(has.sum())
        assert np.array_equal(goals[has], want_goal[has]), s
        assert np.isnan(goals[(want_index < 0) & sure[:, None]]).all(), s
        if has.any():
            worst = max(worst, float(np.abs(action - expect)[has].max()))
            assert worst < 1e-9, (s, worst)
        none = (want_index < 0) & sure[:, None]
        same = (action == prev).all(axis=-1)
        inside = (np.abs(action[..., 0]) <= rot) & (np.abs(action[..., 1]) <= zoom)
        assert (same | inside)[none].all(), s
        kept += int((same & none).sum())
        resampled += int((~same & none).sum())
        prev = action.copy()
    print(config, n, 'camera-steps', camera_steps, 'excused', excused, 'environment-steps with a decision within 1e-9 of a tie', near, 'with a goal', with_goal, 'kept', kept, 'resampled', resampled,
          'worst action difference', worst, 'restarts', restarts)
    assert excused <= 0.001 * camera_steps, (excused, camera_steps)
    assert with_goal > 0
    if shipped and Nc > 2:
        assert kept > 0 and resampled > 0, (kept, resampled)
    if 'max_episode_steps' in kw:
        assert restarts >= 3 * n      # the first call and two restarts of every environment


def test_batched_restarts_and_graph_replay():
    """auto_reset = 4 over episodes of 25 steps: an environment that idles (done = 2) until the interval's restart keeps its rows; the
    graph stepper's replay of whole intervals equals the direct calls bit for bit."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-4v8-9.yaml', max_episode_steps=25)
    n, k = 64, 4
    direct, graphed = Engine(cfg, n, seed=9), Engine(cfg, n, seed=9)
    for eng in (direct, graphed):
        eng.enable_policies(camera_agent='heuristic')
        eng.reset()
    mine = [torch.zeros((n, eng.num_targets, 2), device=eng.device) for eng in (direct, graphed)]
    counters = [torch.zeros((), device=direct.device) for _ in range(2)]

    def policy(i):
        def between():
            counters[i].add_(1.0)
            mine[i].copy_((torch.sin(counters[i]) * 15.0).expand_as(mine[i]))
        return between

    stepper = graphed.make_stepper(None, mine[1], auto_reset=k, graph_steps=2 * k, between=policy(1), versus='target')
    assert stepper.graph is not None
    total = stepper.warmup_steps + 5 * 2 * k      # ten restart intervals behind the warm-up one: episodes end at step 25
    idle_rows = 0
    before = None
    for s in range(total):
        policy(0)()
        direct.step_versus_greedy('target', mine[0], auto_reset=k)
        assert direct.last_flow not in ONE_LAUNCH_FLOWS
        rows = (direct.policy_actions()[0],) + direct.heuristic_camera_goals()
        idle = direct.scalars[:, 2] == 2
        if before is not None:
            for a, b in zip(rows, before):
                assert torch.equal(a[idle].view(torch.uint8), b[idle].view(torch.uint8)), s
        idle_rows += int(idle.sum())
        before = rows
    assert idle_rows > 0
    for _ in range(5):
        stepper.run(2 * k)
    for a, b in ((direct.scalars, graphed.scalars), (direct.masks, graphed.masks), (direct.camera_obs, graphed.camera_obs), (direct.target_obs, graphed.target_obs),
                 (direct.export_state(), graphed.export_state())):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for a, b in zip(direct.policy_actions() + direct.heuristic_camera_goals(), graphed.policy_actions() + graphed.heuristic_camera_goals()):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    stepper.close()
    assert (direct.state_dict()['episode'] >= 2).all()


def test_greedy_is_untouched_by_the_switch():
    """An engine that switched to Heuristic and back -- before the first step and again in the middle -- is bit-identical to one that never
    did, and runs the one-launch form again."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-4v8-9.yaml', max_episode_steps=30)
    n = 96
    plain, switched = Engine(cfg, n, seed=3), Engine(cfg, n, seed=3)
    for eng in (plain, switched):
        eng.enable_policies()
        eng.reset()
    switched.set_camera_opponent('heuristic')
    switched.set_camera_opponent('greedy')
    gen = torch.Generator(device='cpu').manual_seed(1)
    mine = torch.zeros((n, plain.num_targets, 2), device=plain.device)
    for s in range(50):
        mine.copy_((torch.rand(mine.shape, generator=gen) * 2.0 - 1.0) * 20.0)
        if s == 25:
            switched.set_camera_opponent('heuristic')
            assert switched.camera_agent == 'heuristic'
            switched.set_camera_opponent('greedy')
        for eng in (plain, switched):
            eng.step_versus_greedy('target', mine, auto_reset=True)
        assert switched.last_flow == plain.last_flow and plain.last_flow in ONE_LAUNCH_FLOWS, s
        for a, b in ((plain.scalars, switched.scalars), (plain.masks, switched.masks), (plain.camera_obs, switched.camera_obs), (plain.target_obs, switched.target_obs)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), s
        assert torch.equal(switched.policy_actions()[0], plain.policy_actions()[0])
    assert torch.equal(plain.export_state(), switched.export_state())


def test_switching_back_after_heuristic_steps_resets_the_greedy_cameras():
    """The Greedy camera agents sit out while the Heuristic ones play; switching back marks them for their reset at their next acting
    call: the engine then equals one whose Greedy cameras start to act at that step of the same episode with fresh memory."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-4v8-9.yaml')
    n = 16
    eng = Engine(cfg, n, seed=4)
    eng.enable_policies()
    eng.reset()
    theirs = torch.zeros((n, eng.num_targets, 2), device=eng.device)
    for _ in range(3):
        eng.step_versus_greedy('target', theirs)          # the Greedy cameras build up memory and a previous action
    eng.set_camera_opponent('heuristic')
    for _ in range(3):
        eng.step_versus_greedy('target', theirs)
        assert eng.last_flow not in ONE_LAUNCH_FLOWS
    eng.set_camera_opponent('greedy')
    fresh = Engine(cfg, n, seed=4)
    fresh.enable_policies()
    fresh.reset()
    fresh.import_state(eng.export_state())
    fresh.observe()
    eng.observe()
    for s in range(5):
        for e in (eng, fresh):
            e.step_versus_greedy('target', theirs)
        assert torch.equal(eng.policy_actions()[0], fresh.policy_actions()[0]), s


def test_refusals_name_the_opponent_and_leave_the_engine_usable():
    from mate_amd._native import EngineError
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-4v8-9.yaml')
    n = 32
    eng = Engine(cfg, n, seed=2)
    with pytest.raises(EngineError, match='policy_enable') as err:
        eng.set_camera_opponent('heuristic')
    assert err.value.code == ESTATE and eng.camera_agent == 'greedy'
    with pytest.raises(ValueError, match='camera_agent'):
        eng.set_camera_opponent('smart')
    with pytest.raises(ValueError, match='camera_agent'):
        eng.enable_policies(camera_agent='smart')
    eng.enable_policies()
    # the C ABI itself, on an engine the Python host has installed no tables in: Heuristic before the tables, a null table, an unknown opponent
    raw = Engine(cfg, 4, seed=2)
    raw.enable_policies()
    assert raw.lib.mate_engine_set_camera_opponent(raw._h, 1) == ESTATE
    assert b'tables' in raw.lib.mate_engine_last_error()
    assert raw.lib.mate_engine_heuristic_camera_tables(raw._h, None, None, None) == EINVAL
    assert raw.lib.mate_engine_set_camera_opponent(raw._h, 2) == EINVAL
    assert raw.lib.mate_engine_heuristic_camera_goals(raw._h, None, None, None) == ESTATE
    assert raw.lib.mate_engine_set_camera_opponent(raw._h, 0) == 0
    eng.set_camera_opponent('heuristic')
    eng.reset()
    theirs = torch.zeros((n, eng.num_targets, 2), device=eng.device)
    mine = torch.zeros((n, eng.num_cameras, 2), device=eng.device)
    before = eng.export_state().clone()
    with pytest.raises(EngineError, match='heuristic') as err:
        eng.rollout_greedy(4)
    assert err.value.code == ESTATE
    with pytest.raises(EngineError, match='heuristic') as err:
        eng.rollout_versus_greedy('target', theirs, 4)
    assert err.value.code == ESTATE
    for mode in ('enhanced', 'shared'):
        with pytest.raises(EngineError, match='heuristic') as err:
            eng.set_obs_mode(camera=mode)
        assert err.value.code == EINVAL
    with pytest.raises(ValueError, match='heuristic'):
        eng.make_stepper(None, theirs, versus='target', frame_skip=4)
    with pytest.raises(ValueError, match='heuristic'):
        eng.make_stepper(None, theirs, versus='target', frame_skip=4, graph_steps=2)
    with pytest.raises(ValueError, match='int8'):
        eng.heuristic_camera_tape(record=torch.zeros((n, 32, eng.num_cameras), dtype=torch.int32, device=eng.device))
    assert torch.equal(before, eng.export_state())      # nothing ran
    # the caller plays the cameras: unaffected, the fused launch included; and the engine steps on
    eng.rollout_versus_greedy('camera', mine, 3)
    eng.step_versus_greedy('camera', mine)
    assert eng.last_flow in ONE_LAUNCH_FLOWS
    for _ in range(3):
        eng.step_versus_greedy('target', theirs)
        assert eng.last_flow not in ONE_LAUNCH_FLOWS
    eng.step_greedy()
    assert eng.last_flow not in ONE_LAUNCH_FLOWS
    # both heuristic opponents together
    eng.set_target_opponent('heuristic')
    eng.step_greedy()
    cam, tgt, greedy = eng.policy_actions(greedy_targets=True)
    goals, index = eng.heuristic_camera_goals()
    assert torch.equal(index >= 0, ~torch.isnan(goals[..., 0]))
    eng.set_target_opponent('greedy')
    # ... and the other way round: Heuristic is refused under a non-plain camera team mode
    eng.set_camera_opponent('greedy')
    eng.set_obs_mode(camera='enhanced')
    with pytest.raises(EngineError, match='plain rows') as err:
        eng.set_camera_opponent('heuristic')
    assert err.value.code == EINVAL and eng.camera_agent == 'greedy'
    eng.set_obs_mode(target='shared')
    eng.set_camera_opponent('heuristic')
    eng.step_greedy()
    # policy_actions is what the LAST step consumed: behind a call in which the caller played the cameras, not the heuristic launch's buffer
    eng.set_obs_mode()
    ones = torch.ones((n, eng.num_cameras, 2), device=eng.device)
    eng.step_versus_greedy('camera', ones)
    assert eng.last_flow in ONE_LAUNCH_FLOWS
    assert torch.equal(eng.policy_actions()[0], ones.double())


def test_a_scenario_without_cameras_is_the_greedy_one():
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config('MATE-Navigation.yaml')
    n = 17
    plain, selected = Engine(cfg, n, seed=6), Engine(cfg, n, seed=6)
    plain.enable_policies()
    selected.enable_policies(camera_agent='heuristic')
    assert selected.camera_agent == 'heuristic' and selected.num_cameras == 0
    for eng in (plain, selected):
        eng.reset()
    for s in range(20):
        for eng in (plain, selected):
            eng.step_greedy(auto_reset=True)
        assert selected.last_flow == plain.last_flow
        for a, b in ((plain.scalars, selected.scalars), (plain.target_obs, selected.target_obs), (plain.masks, selected.masks),
                     (plain.export_state(), selected.export_state())):
            assert torch.equal(a, b), s
    selected.rollout_greedy(4)      # (nobody to play: the fused launches stay available)


def test_one_camera_is_the_controller_alone():
    import shape_edges
    from mate_amd.engine import Engine
    cfg = shape_edges.scenario((1, 4, 0))      # (the targets start beside the camera)
    n = 9
    eng = Engine(cfg, n, seed=8)
    eng.enable_policies(camera_agent='heuristic')
    eng.reset()
    cam = U.scenario_tables(cfg)['camera']
    used = torch.full((n, 32, 1), -1, dtype=torch.int8, device=eng.device)
    eng.heuristic_camera_tape(record=used)
    prev = np.zeros((n, 1, 2))
    compared = 0
    for s in range(10):
        sd = eng.state_dict()
        seen = eng.unpack_masks()['camera_target_view_mask']
        eng.step_greedy(auto_reset=True)
        assert (used == 0).all()
        action = eng.policy_actions()[0].cpu().numpy()
        index = eng.heuristic_camera_goals()[1].cpu().numpy()
        expect, want_index, _, info = heuristic_cameras(
            cam_xy=np.stack([sd['cam_x'], sd['cam_y']], axis=-1), cam_phi=sd['cam_phi'], cam_theta=sd['cam_theta'],
            tgt_xy=np.stack([sd['tgt_x'], sd['tgt_y']], axis=-1), seen=seen, permutations=used.cpu().numpy(), prev_action=prev,
            binom_u=np.zeros((n, 1)), sample_u=np.zeros((n, 1, 2)), rot=cam['rotation_step'], zoom=cam['zooming_step'], rmax=cam['max_sight_range'],
            tables=_tables(cfg))
        sure = info['margins']['range'] > 1e-9      # (as in the batch test)
        assert np.array_equal(index[sure], want_index[sure]), s
        has = (want_index >= 0) & sure[:, None]
        assert np.abs(action - expect)[has].max(initial=0.0) < 1e-9
        compared += int(has.sum())
        prev = action.copy()
    assert compared > 0


def test_entry_points_take_the_camera_agent(monkeypatch, capsys):
    import mate_amd
    import mate_amd.evaluate as E
    env = mate_amd.BatchedMultiAgentTracking('MATE-4v2-9.yaml', num_envs=8, camera_agent='heuristic', max_episode_steps=6)
    env.reset()
    assert env.engine.camera_agent == 'heuristic'
    for _ in range(6):
        env.step_versus_greedy('target', torch.zeros((8, env.num_targets, 2), device=env.device))
        assert env.engine.last_flow not in ONE_LAUNCH_FLOWS
    single = mate_amd.MultiAgentTracking('MATE-4v2-9.yaml')
    single.enable_greedy_policies(camera_agent='heuristic')
    single.seed(0)
    single.reset()
    single.step_greedy()
    assert single.engine.camera_agent == 'heuristic'
    monkeypatch.setattr('sys.argv', ['evaluate', '--config', 'MATE-4v2-9.yaml', '--camera-agent', 'heuristic', '--max-episode-steps', '8'])
    rows = E.main()
    assert len(rows) == 1
    assert 'episode 0' in capsys.readouterr().out
