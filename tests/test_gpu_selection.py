"""Target-selection camera actions on the device (Engine.enable_selection / step_selected; csrc/selection_rows.hpp) against the
reference's HierarchicalCamera wrapper (examples/hrl/wrappers.py): the recorded fixtures replayed with their tapes, the fragment that
ends an episode, batches that do not fill their tiles, graph replay, the launch order with state and reward rows attached, the team
observation modes, the error paths (the kernels' resources: tests/test_kernel_resources.py).  Executor actions: 1e-9 absolute (the project's bar for f64 positions
and angles); masks, rewards, done, integer metrics, the rate (one IEEE division of small integers) and the
action mask: exact."""
import os

import numpy as np
import pytest
import torch

import golden_util as G
import gpu_util as U
from test_selection_host import FIXTURES, action_mask_numpy, camera_constants, metrics_numpy, track_numpy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9


def _tapes(fx, s, N, dev):
    def bc(a, dtype=np.float64):
        a = np.asarray(a)
        return torch.from_numpy(np.broadcast_to(a, (N,) + a.shape).astype(dtype).copy()).to(dev)

    def draws(key, shape):             # the greedy targets' recorded draws; the learner's team has no agents: zeros
        return bc(np.nan_to_num(fx['step/' + key][s], nan=0.0)) if 'step/' + key in fx else bc(np.zeros(shape))
    Nc, Nt = int(fx['num_cameras']), int(fx['num_targets'])
    policy = {
        'camera_resample_u': bc(np.zeros(Nc)), 'camera_sample_u': bc(np.zeros((Nc, 2))), 'camera_delay': bc(np.full((Nc, Nc), -1), np.int32),
        'target_choice_u': draws('agent_tgt_choice_u', Nt), 'target_resample_u': draws('agent_tgt_binom_u', Nt),
        'target_sample_u': draws('agent_tgt_sample_u', (Nt, 2)), 'target_reset_sample_u': bc(fx['agent/tgt_reset_sample_u']),
    }
    return policy, bc(np.nan_to_num(fx['step/tape_ct'][s], nan=0.0)), bc(np.nan_to_num(fx['step/goal_u'][s], nan=0.0))


def _words(bits):
    return (np.asarray(bits).astype(np.int64) << np.arange(bits.shape[-1])).sum(axis=-1).astype(np.int32)


@pytest.mark.parametrize('obs_dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_replay_and_fragment_end(name, obs_dtype):
    """Every fixture through step_selected with its tapes.  frame_skip = K > 1 runs whole fragments under the batched restart K: the
    environment that finishes inside its fragment (selection_2v4-0_multi_s33) adds nothing after its terminal frame, restarts behind
    the fragment and shows the new episode's view in its action-mask row."""
    from mate_amd.engine import Engine
    fx = G.load(name + '.npz')
    N, K, multi = 2, int(fx['frame_skip']), bool(fx['multi_selection'])
    Nc, Nt = int(fx['num_cameras']), int(fx['num_targets'])
    eng = U.load_fixture_state(Engine(U.config_of_fixture(fx), N, seed=5, obs_dtype=obs_dtype), fx)
    eng.enable_policies()
    dev = eng.device
    tape0 = torch.from_numpy(np.where(fx['reset/camera_target_view_mask'], 1.0, 0.0)[None].repeat(N, 0)).to(dev)
    eng.observe(tape_ct=tape0)
    assert np.array_equal(eng.unpack_masks()['camera_target_view_mask'][0], fx['reset/camera_target_view_mask'])
    shaped = 'aux_keys' in fx
    if shaped:
        eng.enable_reward_rows(camera=(dict(zip((str(k) for k in fx['aux_keys']), (float(c) for c in fx['aux_coefficients']))), str(fx['aux_reduction'])))
    eng.enable_selection(multi)
    assert np.array_equal(eng.action_mask[1].cpu().numpy(), fx['reset/action_mask'])
    T = len(fx['step/done'])
    s = 0
    for ls, frames in enumerate(fx['skip/frames']):
        sel = fx['skip/selection'][ls]
        eng.selection.copy_(eng.encode_selection(torch.from_numpy(np.broadcast_to(sel, (N,) + sel.shape).copy()), multi))
        if multi:
            assert np.array_equal(eng.selection[0].cpu().numpy(), _words(fx['skip/selection_bits'][ls]))
        executed, metric_sum, reward_sum = 0, np.zeros((Nc, 4)), np.zeros(Nc)
        for f in range(K):
            live = f < frames
            policy, tape_ct, tape_goal = _tapes(fx, s if live else T - 1, N, dev)
            eng.step_selected(policy_tape=policy, tape_ct=tape_ct, tape_goal=tape_goal, auto_reset=K if K > 1 else False)
            n = eng.selection_frames.cpu().numpy()
            assert (n == int(live)).all(), (ls, f, n)
            executed += int(n[0])
            metrics = eng.selection_metrics[1].cpu().numpy()
            if not live:                               # idle behind its terminal frame: nothing is added
                assert float(eng.scalars[0, 2]) == 2.0 and not metrics.any()
                continue
            err = np.abs(eng.selection_actions[0].double().cpu().numpy() - fx['step/executor_act'][s]).max()
            print(f'{name} frame {s}: executor error {err:.3e}')
            assert err <= TOL, (s, err)
            terminal = bool(fx['step/done'][s])
            if not (terminal and f == K - 1):          # (the restart behind a fragment's last frame rewrites the masks)
                assert np.array_equal(eng.unpack_masks()['camera_target_view_mask'][1], fx['step/view_after'][s]), s
            assert float(eng.scalars[0, 0]) == np.float32(fx['step/reward_cam'][s]), s
            assert bool(eng.scalars[1, 2] == 1) == terminal, s
            assert np.array_equal(metrics, fx['step/metrics'][s]), s
            metric_sum += metrics
            if shaped:
                rows = eng.camera_reward_rows[0].cpu().numpy()
                np.testing.assert_allclose(rows, fx['step/shaped_reward_cam'][s], rtol=0, atol=1e-6, err_msg=str(s))
                reward_sum += rows
            else:
                reward_sum += float(eng.scalars[0, 0])
            s += 1
        assert executed == frames, (ls, executed, frames)
        np.testing.assert_allclose(reward_sum, fx['skip/reward_cam'][ls], rtol=1e-6, atol=5e-6)
        if K > 1:
            np.testing.assert_allclose(metric_sum / frames, fx['skip/info_metrics'][ls], rtol=0, atol=1e-12)
        view = eng.unpack_masks()['camera_target_view_mask']
        assert np.array_equal(eng.action_mask.cpu().numpy(), action_mask_numpy(view, multi))
        if not bool(fx['skip/done'][ls]):
            assert np.array_equal(eng.action_mask[0].cpu().numpy(), fx['skip/action_mask'][ls]), ls
        elif K > 1:                                    # restarted behind the fragment: a new episode, its first view
            sd = eng.state_dict()
            assert (sd['episode'] == 2).all() and (sd['episode_step'] == 0).all() and (sd['done'] == 0).all()
    assert s == T


@pytest.mark.parametrize('name', [n for n in FIXTURES if n != 'selection_4v8-9_multi_s31'])
def test_accumulated_fragments_are_the_wrappers_means(name):
    """The frame_skip > 1 fixtures with enable_selection(accumulate=True): metrics += and frames += 1 per executed frame, an idle
    environment adds nothing, so selection_metrics / selection_frames is the wrapper's mean (skip/info_metrics) and selection_frames
    its executed frame count (skip/frames) -- against the reference's record, not against the overwrite mode."""
    from mate_amd.engine import Engine
    fx = G.load(name + '.npz')
    N, K, multi = 2, int(fx['frame_skip']), bool(fx['multi_selection'])
    eng = U.load_fixture_state(Engine(U.config_of_fixture(fx), N, seed=5, obs_dtype=torch.float64), fx)
    eng.enable_policies()
    dev = eng.device
    eng.observe(tape_ct=torch.from_numpy(np.where(fx['reset/camera_target_view_mask'], 1.0, 0.0)[None].repeat(N, 0)).to(dev))
    eng.enable_selection(multi, accumulate=True)
    T, s = len(fx['step/done']), 0
    for ls, frames in enumerate(fx['skip/frames']):
        sel = fx['skip/selection'][ls]
        eng.selection.copy_(eng.encode_selection(torch.from_numpy(np.broadcast_to(sel, (N,) + sel.shape).copy()), multi))
        eng.selection_metrics.zero_()
        eng.selection_frames.zero_()
        for f in range(K):
            policy, tape_ct, tape_goal = _tapes(fx, s if f < frames else T - 1, N, dev)
            eng.step_selected(policy_tape=policy, tape_ct=tape_ct, tape_goal=tape_goal, auto_reset=K)
            s += int(f < frames)
        n = eng.selection_frames.cpu().numpy()
        assert (n == frames).all(), (ls, n, frames)
        mean = (eng.selection_metrics / eng.selection_frames.double()[:, None, None]).cpu().numpy()
        np.testing.assert_allclose(mean[0], fx['skip/info_metrics'][ls], rtol=0, atol=1e-12, err_msg=str(ls))
        assert np.array_equal(mean[0], mean[1])
    assert s == T


@pytest.mark.parametrize('name', FIXTURES)
def test_environment_class_replays_the_fixture(name):
    """BatchedMultiAgentTracking(camera_selection=...): step_selected / selection_info / action_mask against the wrapper's record.
    frame_skip = K > 1 is K calls with the selection held in an environment built with auto_reset = K; the caller adds the rewards
    and metrics of the frames that ran (selection_info()['frames'])."""
    from mate_amd.environment import BatchedMultiAgentTracking
    fx = G.load(name + '.npz')
    N, K, multi = 2, int(fx['frame_skip']), bool(fx['multi_selection'])
    Nc = int(fx['num_cameras'])
    shaped = 'aux_keys' in fx
    shaping = (dict(zip((str(k) for k in fx['aux_keys']), (float(c) for c in fx['aux_coefficients']))), str(fx['aux_reduction'])) if shaped else None
    env = BatchedMultiAgentTracking(U.config_of_fixture(fx), num_envs=N, seed=5, obs_dtype=torch.float64, auto_reset=K if K > 1 else False,
                                    camera_selection='multi' if multi else 'single', camera_reward_shaping=shaping)
    env.reset()
    eng, dev = env.engine, env.device
    view = eng.unpack_masks()['camera_target_view_mask']
    assert np.array_equal(env.action_mask().cpu().numpy(), action_mask_numpy(view, multi))
    env.reset()                                        # (a second reset: the mask follows the new first view)
    assert np.array_equal(env.action_mask().cpu().numpy(), action_mask_numpy(eng.unpack_masks()['camera_target_view_mask'], multi))
    U.load_fixture_state(eng, fx)
    eng.observe(tape_ct=torch.from_numpy(np.where(fx['reset/camera_target_view_mask'], 1.0, 0.0)[None].repeat(N, 0)).to(dev))
    assert np.array_equal(env.action_mask()[1].cpu().numpy(), fx['reset/action_mask'])      # (... and observe())
    T, s = len(fx['step/done']), 0
    for ls, frames in enumerate(fx['skip/frames']):
        sel = torch.from_numpy(np.broadcast_to(fx['skip/selection'][ls], (N,) + fx['skip/selection'][ls].shape).copy())
        reward_sum, metric_sum, executed = np.zeros(Nc), np.zeros((Nc, 4)), 0
        for f in range(K):
            policy, tape_ct, tape_goal = _tapes(fx, s if f < frames else T - 1, N, dev)
            (cam_obs, tgt_obs), (reward_cam, _), done, info = env.step_selected(sel, policy_tape=policy, tape_ct=tape_ct, tape_goal=tape_goal)
            sinfo = env.selection_info()
            ran = int(sinfo['frames'][0])
            assert ran == int(f < frames) and (sinfo['frames'] == ran).all(), (ls, f)
            if not ran:
                assert bool(done.all()) and not any(bool(sinfo[k].any()) for k in eng.SELECTION_METRICS)
                continue
            assert float(reward_cam[0]) == np.float32(fx['step/reward_cam'][s]) and bool(done[1]) == bool(fx['step/done'][s]), s
            metrics = np.stack([sinfo[k][1].cpu().numpy() for k in eng.SELECTION_METRICS], axis=-1)
            assert np.array_equal(metrics, fx['step/metrics'][s]), s
            metric_sum += metrics
            reward_sum += env.shaped_rewards()[0][0].cpu().numpy() if shaped else float(reward_cam[0])
            executed += 1
            s += 1
        assert executed == frames
        np.testing.assert_allclose(reward_sum, fx['skip/reward_cam'][ls], rtol=1e-6, atol=5e-6)
        np.testing.assert_allclose(metric_sum / frames, fx['skip/info_metrics'][ls], rtol=0, atol=1e-12)
        assert cam_obs is eng.camera_obs
        if not bool(fx['skip/done'][ls]):
            assert np.array_equal(env.action_mask()[0].cpu().numpy(), fx['skip/action_mask'][ls]), ls
        elif K > 1:                                    # restarted behind the fragment: the new episode's first view
            assert (eng.state_dict()['episode_step'] == 0).all()
            assert np.array_equal(env.action_mask().cpu().numpy(), action_mask_numpy(eng.unpack_masks()['camera_target_view_mask'], multi))
    assert s == T


def test_f32_joint_action():
    """enable_selection(act_dtype=torch.float32): selection_kernel<float> writes f32 pairs and the stepping launch reads them as such.
    The executor against the NumPy restatement at 1e-9 plus one f32 rounding of the value (|a| 2^-24); the cameras then move by
    exactly the f32 action (Camera.simulate adds the clipped action to orientation and viewing angle)."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    n = 40
    eng = Engine(read_config('MATE-4v8-9.yaml'), n, seed=13)
    eng.enable_policies()
    eng.reset()
    eng.enable_selection(True, act_dtype=torch.float32)
    assert eng.selection_actions.dtype == torch.float32 and eng.selection_actions.shape == (n, eng.num_cameras, 2)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(5)
    consts = _constants_of(eng)
    for step in range(3):
        eng.selection.copy_(torch.randint(0, 256, (n, eng.num_cameras), device='cuda', generator=gen, dtype=torch.int32))
        sd = eng.state_dict()
        view = eng.unpack_masks()['camera_target_view_mask']
        expect, margins = _track_batch(sd, view, _bits_of(eng.selection.cpu().numpy(), eng.num_targets), consts)
        eng.step_selected(auto_reset=False)
        got = eng.selection_actions.cpu().numpy()
        use = margins >= 1e-9
        assert use.mean() >= 0.999
        assert (np.abs(got.astype(np.float64) - expect)[use] <= TOL + np.abs(expect[use]) * 2.0 ** -24).all()
        after = eng.state_dict()
        moved = (after['cam_phi'] - sd['cam_phi'] + 180.0) % 360.0 - 180.0
        assert np.abs(moved - got[..., 0].astype(np.float64)).max() <= 1e-9
    assert (np.abs(got[..., 0]) > 0).any()


def _track_batch(sd, view, sel, c):
    """track_numpy over a batch: sd = Engine.state_dict(), view / sel [N, Nc, Nt] bool -> (actions [N, Nc, 2], margins [N, Nc])."""
    valid = sel & view
    n = valid.sum(axis=-1)
    cx = np.zeros(n.shape)
    cy = np.zeros(n.shape)
    for t in range(valid.shape[-1]):                   # the rows added in target order
        cx = np.where(valid[:, :, t], cx + sd['tgt_x'][:, None, t], cx)
        cy = np.where(valid[:, :, t], cy + sd['tgt_y'][:, None, t], cy)
    some = n > 0
    nn = np.maximum(n, 1)
    dx, dy = cx / nn - sd['cam_x'], cy / nn - sd['cam_y']
    orientation = np.rad2deg(np.arctan2(dy, dx))
    distance = np.sqrt(dx * dx + dy * dy)
    theta = sd['cam_theta']
    area_product = theta * np.square(np.sqrt(c['area'] / theta))
    reach = distance * (1.0 + np.sin(np.deg2rad(c['min_viewing_angle'] / 2.0)))
    near = np.sqrt(area_product / 180.0) / 2.0
    margins = np.where(some, np.minimum(np.abs(reach - c['max_sight_range']) / c['max_sight_range'], np.abs(distance - near) / near), np.inf)
    best = np.full(n.shape, 180.0)
    d = np.where(some, distance, 1.0)
    for _ in range(20):
        best = area_product / np.square(d * (1.0 + np.sin(np.deg2rad(np.minimum(best / 2.0, 90.0)))))
    best = np.clip(best, c['min_viewing_angle'], 180.0)
    best = np.where(reach >= c['max_sight_range'], c['min_viewing_angle'], np.where(distance <= near, 180.0, best))
    a0 = np.clip((orientation - sd['cam_phi'] + 180.0) % 360.0 - 180.0, -c['rotation_step'], c['rotation_step'])
    a1 = np.clip(best - theta, -c['zooming_step'], c['zooming_step'])
    actions = np.stack([np.where(some, a0, -c['rotation_step']), np.where(some, a1, -c['zooming_step'])], axis=-1)
    return actions, margins


def _constants_of(eng):
    cam = {key: value for key, value in U.scenario_tables(eng.config)['camera'].items() if key != 'radius'}
    return dict(cam, area=cam['min_viewing_angle'] * np.square(cam['max_sight_range']))


def _bits_of(words, Nt):
    return ((words[..., None] >> np.arange(Nt)) & 1).astype(bool)


@pytest.mark.parametrize('config,n', [('MATE-4v8-9.yaml', 272), ('MATE-2v4-0.yaml', None)])
def test_batches_that_do_not_fill_their_tiles(config, n):
    """272 environments: neither a multiple of 16 nor of 256.  MATE-2v4-0: one environment more than 32 per compute unit (the
    threshold of sub_wave_of_launch, csrc/engine_host.h), so the sub-wave per-step plan is in force, and no multiple of 16.  Philox
    draws, random selections, 12 steps; the executor against the NumPy restatement on the state exported before each step.  A
    camera-frame is left out only if its branch margin, computed by the NumPy side, is below 1e-9 relative: at most 0.1 % of them."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    if n is None:
        n = 32 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    eng = Engine(read_config(config), n, seed=41)
    eng.enable_policies()
    eng.reset()
    eng.enable_selection(True)
    Nc, Nt = eng.num_cameras, eng.num_targets
    consts = _constants_of(eng)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(7)
    left_out, total, worst = 0, 0, 0.0
    for step in range(12):
        keep = torch.rand((n, Nc, Nt), device='cuda', generator=gen) < 0.45
        eng.selection.copy_(eng.encode_selection(keep.to(torch.int32)))
        sd = eng.state_dict()
        view = eng.unpack_masks()['camera_target_view_mask']
        sel = _bits_of(eng.selection.cpu().numpy(), Nt)
        assert np.array_equal(sel, keep.cpu().numpy())
        expect, margins = _track_batch(sd, view, sel, consts)
        if step == 0:                                  # the batch form is the per-environment form
            for e in range(0, n, max(1, n // 16)):
                one, _ = track_numpy(np.stack([sd['cam_x'][e], sd['cam_y'][e]], axis=-1), sd['cam_phi'][e], sd['cam_theta'][e],
                                     np.stack([sd['tgt_x'][e], sd['tgt_y'][e]], axis=-1), sel[e], view[e], **consts)
                assert np.abs(one - expect[e]).max() <= 1e-12
        eng.step_selected(auto_reset=True)
        got = eng.selection_actions.cpu().numpy()
        use = margins >= 1e-9
        left_out += int((~use).sum())
        total += use.size
        worst = max(worst, float(np.abs(got - expect)[use].max()))
        alive = eng.scalars[:, 2].cpu().numpy() != 2
        after = eng.unpack_masks()['camera_target_view_mask']
        fresh = eng.scalars[:, 2].cpu().numpy() == 1   # (restarted inside the call: the masks are the new episode's)
        assert np.array_equal(eng.selection_metrics.cpu().numpy()[alive & ~fresh], metrics_numpy(sel, after)[alive & ~fresh])
        assert np.array_equal(eng.action_mask.cpu().numpy(), action_mask_numpy(after, True))
    print(f'{config} x {n}: worst executor error {worst:.3e}, {left_out} of {total} camera-frames left out')
    assert worst <= TOL, worst
    assert left_out <= 0.001 * total, (left_out, total)


def test_graph_replay_of_fragments_is_five_direct_calls():
    """make_stepper(versus='selection', frame_skip=5) in a graph against five direct step_selected calls under the batched restart 5:
    rows, scalars, metrics, frames and accumulated reward rows bit for bit."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg, n, K = read_config('MATE-4v8-9.yaml', max_episode_steps=12), 272, 5
    a, b = (Engine(cfg, n, seed=23) for _ in range(2))
    for e in (a, b):
        e.enable_policies()
        e.reset()
        e.enable_reward_rows(camera=({'coverage_rate': 1.0}, 'mean'), accumulate=True)
        e.enable_selection(True, accumulate=True)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(11)

    def direct():
        b.selection_metrics.zero_(); b.selection_frames.zero_(); b.camera_reward_rows.zero_()
        for _ in range(K):
            b.step_selected(auto_reset=K)

    stepper = a.make_stepper(None, None, auto_reset=True, graph_steps=1, versus='selection', frame_skip=K)
    direct()                                           # (the stepper's warm-up fragment)
    finished = 0
    for fragment in range(4):
        sel = torch.randint(0, 256, (n, a.num_cameras), device='cuda', generator=gen, dtype=torch.int32)
        a.selection.copy_(sel); b.selection.copy_(sel)
        stepper.run(1)
        direct()
        for key in ('camera_obs', 'target_obs', 'scalars', 'masks', 'selection_metrics', 'selection_frames', 'selection_actions', 'camera_reward_rows', 'action_mask'):
            assert torch.equal(getattr(a, key), getattr(b, key)), (fragment, key)
        finished += int((a.selection_frames < K).sum())
    assert finished > 0                                # (12-step episodes: environments did finish inside fragments)
    stepper.close()
    assert torch.equal(a.export_state(), b.export_state())


def test_order_with_state_and_reward_rows_attached():
    """Reward and metric rows describe the terminal step; state and action-mask rows describe the restarted episode."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg, n = read_config('MATE-2v4-0.yaml', max_episode_steps=4), 48
    a, b = (Engine(cfg, n, seed=3) for _ in range(2))
    for e in (a, b):
        e.enable_policies()
        e.reset()
        e.enable_state_rows()
        e.enable_reward_rows(camera=({'coverage_rate': 1.0, 'num_tracked': 0.5}, 'none'))
        e.enable_selection(True)
        e.selection.fill_(0b1011)
    episode = a.state_dict()['episode'].copy()
    terminal = False
    for step in range(6):
        a.step_selected(auto_reset=True)
        b.step_selected(auto_reset=False)
        terminal = bool((b.scalars[:, 2] == 1).all())
        assert torch.equal(a.scalars, b.scalars)
        # the step's own rows: the same with and without the restart behind them
        assert torch.equal(a.camera_reward_rows, b.camera_reward_rows) and torch.equal(a.selection_metrics, b.selection_metrics)
        assert np.array_equal(b.selection_metrics.cpu().numpy(), metrics_numpy(_bits_of(b.selection.cpu().numpy(), 4), b.unpack_masks()['camera_target_view_mask']))
        if terminal:
            break
    assert terminal
    sd = a.state_dict()
    assert (sd['episode'] == episode + 1).all() and (sd['episode_step'] == 0).all()
    assert torch.equal(a.state, a.state_rows()) and not torch.equal(a.state, b.state)
    assert np.array_equal(a.action_mask.cpu().numpy(), action_mask_numpy(a.unpack_masks()['camera_target_view_mask'], True))
    assert np.array_equal(b.action_mask.cpu().numpy(), action_mask_numpy(b.unpack_masks()['camera_target_view_mask'], True))


@pytest.mark.parametrize('mode', ['shared', 'enhanced'])
def test_team_observation_modes_act_on_the_flag_column(mode):
    """SharedFieldOfView / EnhancedObservation of the camera team: valid = selection & the opponent-flag column of camera_obs."""
    from mate_amd import constants as consts
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    eng = Engine(read_config('MATE-4v8-9.yaml'), 40, seed=9, obs_dtype=torch.float64)
    eng.set_obs_mode(camera=mode)
    eng.enable_policies()
    eng.reset()
    eng.enable_selection(True)
    Nc, Nt = eng.num_cameras, eng.num_targets
    column = consts.camera_observation_slices_of(Nc, Nt, eng.num_obstacles)['opponent_mask']
    gen = torch.Generator(device='cuda')
    gen.manual_seed(2)
    for step in range(3):
        eng.selection.copy_(torch.randint(0, 256, (40, Nc), device='cuda', generator=gen, dtype=torch.int32))
        flags = eng.camera_obs[:, :, column].cpu().numpy() != 0
        if mode == 'enhanced':
            assert flags.all()
        else:
            assert np.array_equal(flags, np.broadcast_to(eng.unpack_masks()['camera_target_view_mask'].any(axis=1, keepdims=True), flags.shape))
        assert np.array_equal(eng.action_mask.cpu().numpy(), action_mask_numpy(flags, True))
        sel = _bits_of(eng.selection.cpu().numpy(), Nt)
        expect, margins = _track_batch(eng.state_dict(), flags, sel, _constants_of(eng))
        eng.step_selected(auto_reset=False)
        assert np.abs(eng.selection_actions.cpu().numpy() - expect)[margins >= 1e-9].max() <= TOL
        after = eng.camera_obs[:, :, column].cpu().numpy() != 0
        assert np.array_equal(eng.selection_metrics.cpu().numpy(), metrics_numpy(sel, after))


def test_error_paths():
    from mate_amd._native import EngineError
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    import ctypes
    eng = Engine(read_config('MATE-4v2-9.yaml'), 8, seed=1)
    with pytest.raises(EngineError, match='policy_enable'):
        eng.enable_selection(False)
    eng.enable_policies()
    with pytest.raises(EngineError, match='before reset'):
        eng.enable_selection(False)
    eng.reset()
    status = eng.lib.mate_engine_enable_selection(eng._h, 0, None, None, None, None, 0)
    assert status != 0 and 'null selection' in eng.lib.mate_engine_last_error().decode()
    io, keep = eng._io()
    status = eng.lib.mate_engine_step_selected(eng._h, ctypes.byref(io), None, 1, eng._stream())
    assert status != 0 and 'enable_selection' in eng.lib.mate_engine_last_error().decode()
    eng.enable_selection(False)
    with pytest.raises(EngineError, match='pipelined'):
        eng.step_selected(auto_reset=Engine.RESET_PIPELINED)
    with pytest.raises(EngineError, match='pipelined'):
        eng.rollout_greedy(2, auto_reset='pipelined')
    with pytest.raises(AssertionError):
        eng.encode_selection(torch.zeros((8, 4), dtype=torch.float32))
    with pytest.raises(AssertionError):
        eng.encode_selection(torch.zeros((8, 3), dtype=torch.int32))
    eng.step_selected()                               # the engine still steps
    eng.disable_selection()
    assert eng.selection is None
