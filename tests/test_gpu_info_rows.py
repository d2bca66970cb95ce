"""GPU (-m gpu): the MoreTrainingInformation rows (csrc/info_rows.hpp, Engine.enable_info_rows) behind every stepping flow.

References, all independent of the kernel: the reference's own per-step arrays in the recorded traces (tests/golden/trace_*.npz), and
tests/info_ref.py -- the NumPy restatement tests/test_info_rows_host.py holds to those traces exactly -- on Engine.state_dict() and
Engine.unpack_masks(), with info_ref.Model keeping the snapshot of goals and episode numbers across calls as the launch must.
Bars: integer-valued columns (goal, individual_done, is_tracked, is_colliding, both camera columns, the cargo row) exact; distances
1e-9 * max(1, |ref|) against the traces (the bar of the f64 observation rows of the same positions) and 1e-9 absolute against the restatement
(the bar tests/test_gpu_reward_rows.py holds the same arithmetic to).  Deliveries come from the traces and from the planted warehouse
scenes of tests/logistics_scenes.py."""
import ctypes

import numpy as np
import pytest
import torch

import golden_util as G
import gpu_util as U
import info_ref as R
import logistics_scenes as LS
import rim_scenes as RS
import shape_edges as S
from test_info_rows_host import GPU_TRACES

pytestmark = pytest.mark.gpu
MATE_EINVAL, MATE_ESTATE = -1, -4
INTEGER_COLUMNS, DISTANCE_COLUMNS = [0, 6, 7, 8], [1, 2, 3, 4, 5]
CUT = 6                # max_episode_steps of the episode-boundary tests: seven-frame episodes


def _rows(eng):
    torch.cuda.synchronize()
    camera = eng.info_camera_rows.cpu().numpy() if eng.info_camera_rows is not None else np.zeros((eng.num_envs, 0, 2))
    return camera, eng.info_target_rows.cpu().numpy(), eng.info_cargo_rows.cpu().numpy()


def _check(eng, model, where, envs=None, tol=1e-9):
    """The attached rows against the model's, on the environments `envs` ([n] bool; default all)."""
    envs = np.ones(eng.num_envs, dtype=bool) if envs is None else envs
    camera, target, cargo = _rows(eng)
    from mate_amd.engine import Engine
    for col in INTEGER_COLUMNS:
        got, ref = target[..., col], model.target[..., col]
        differs = ~((got == ref) | (np.isnan(got) & np.isnan(ref))) & envs[:, None]
        assert not differs.any(), (where, Engine.INFO_TARGET_COLUMNS[col], [(e, t, got[e, t], ref[e, t]) for e, t in np.argwhere(differs)[:4].tolist()])
    err = np.abs(target[envs][..., DISTANCE_COLUMNS] - model.target[envs][..., DISTANCE_COLUMNS])
    assert err.size == 0 or float(err.max()) <= tol, (where, 'distances', float(err.max()))
    assert np.array_equal(camera[envs], model.camera[envs], equal_nan=True), (where, 'camera rows')
    assert np.array_equal(cargo[envs], model.cargo[envs]), (where, 'cargo rows')
    return float(err.max()) if err.size else 0.0


def _attach(eng):
    eng.enable_info_rows()
    return R.Model(eng.state_dict(), eng.num_cameras)


def _stepped(eng, model, frames=1, masks=None, scalars=None):
    """Behind a stepping call with auto_reset = 0 (the state is still the one the launch saw): the model follows."""
    torch.cuda.synchronize()
    scalars = eng.scalars if scalars is None else scalars
    return model.step(eng.state_dict(), eng.unpack_masks(masks=masks) if masks is not None else eng.unpack_masks(), scalars[:, 2].cpu().numpy(), frames)


# ---------------------------------------------------------------------------------------------- 1: the recorded traces
@pytest.mark.parametrize('name', GPU_TRACES)
def test_rows_on_the_recorded_traces(name):
    """The reference's actions and tapes replayed as tests/test_gpu_parity.py does, three environments, auto_reset = 0: at every step the
    rows against the fixture's own arrays."""
    from test_gpu_parity import _replay
    fx = G.load(name + '.npz')
    N = 3
    eng = U.engine_from_fixture(fx, N, obs_dtype=torch.float64)
    eng.enable_info_rows()
    Nc = eng.num_cameras
    worst, deliveries = 0.0, 0
    for s in range(len(fx['step/done'])):
        _replay(eng, fx, s, N)
        camera, target, cargo = _rows(eng)
        ct, tc = np.asarray(fx['step/camera_target_view_mask'][s]), np.asarray(fx['step/target_camera_view_mask'][s])
        goals = np.asarray(fx['step/tgt_goals'][s])
        wd = np.maximum(np.asarray(fx['step/target_warehouse_distances'][s]) - 75.0, 0.0)
        goal_distance = np.where(goals >= 0, wd[np.arange(len(goals)), np.maximum(goals, 0)], 1000.0)
        remaining = np.asarray(fx['step/remaining_cargoes'][s])
        for e in range(N):
            assert np.array_equal(target[e, :, 0], goals), (s, e, 'goal')
            assert np.array_equal(target[e, :, 6], np.asarray(fx['step/target_dones'][s]).astype(np.float64)), (s, e, 'individual_done')
            assert np.array_equal(target[e, :, 8], np.asarray(fx['step/tgt_colliding'][s]).astype(np.float64)), (s, e, 'is_colliding')
            if Nc:
                assert np.array_equal(target[e, :, 7], ct.any(axis=0)), (s, e, 'is_tracked')
                assert np.array_equal(camera[e, :, 0], ct.sum(axis=1)) and np.array_equal(camera[e, :, 1], tc.any(axis=0)), (s, e, 'camera rows')
            else:
                assert not target[e, :, 7].any()
            assert np.array_equal(cargo[e, 0:4], remaining.sum(axis=-1)) and np.array_equal(cargo[e, 4:8], fx['step/awaiting_cargo_counts'][s]), (s, e, 'cargo counts')
            assert np.array_equal(cargo[e, 8:24], remaining.reshape(16)), (s, e, 'remaining_cargoes')
            for got, ref, what in ((target[e, :, 2:6], wd, 'warehouse_distances'), (target[e, :, 1], goal_distance, 'goal_distance')):
                err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
                worst = max(worst, float(err.max()))
                assert float(err.max()) <= 1e-9, (s, e, what, float(err.max()))
        deliveries += int(np.asarray(fx['step/target_dones'][s]).sum())
    print(f'{name}: {len(fx["step/done"])} steps, {deliveries} deliveries, worst distance error {worst:.3e} of max(1, |ref|)')


# ---------------------------------------------------------------------------------------------- 2: edge shapes on the engine's own draws
EDGE_SHAPES = [S.case_id(c) for c in S.ATTACHED_CASES] + ['MATE-8v8-9 x 65', 'MATE-4v8-9 x 1', 'MATE-4v8-9 x 16', 'MATE-4v8-9 x 17']


@pytest.mark.parametrize('scenario', EDGE_SHAPES)
def test_rows_equal_the_restatement_on_the_engines_own_draws(scenario):
    """Four step_greedy(auto_reset = 0) steps against info_ref on state_dict() / unpack_masks(): the attached cases of tests/shape_edges.py
    (camera -> target rows AND target rows that cross 32-bit words at odd bits, no cameras, 16 x 16 x 64 whose target rows span 48 words),
    65 environments of MATE-8v8-9 (five tiles, the last one of one environment), MATE-4v8-9 at one environment, one full tile and one
    more.  16v16-64 steps under the random policy: no test of the suite runs the on-device agents among 64 obstacles."""
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    if ' x ' in scenario:
        config, n = scenario.split(' x ')
        eng = Engine(read_config(config + '.yaml'), int(n), seed=51)
        greedy = True
    else:
        case = S.attached_case(scenario)
        eng = Engine(S.case_scenario(case), case.n, seed=case.seed, first_env_index=case.first)
        assert not eng.specialised and (eng.num_cameras, eng.num_targets, eng.num_obstacles) == case.shape
        greedy = case.shape != (16, 16, 64)
    if greedy:
        eng.enable_policies()
    eng.reset()
    model = _attach(eng)
    Nc, Nt = eng.num_cameras, eng.num_targets
    assert (eng.info_camera_rows is None) == (Nc == 0)
    straddling = {c: 0 for c in S.straddling_rows(Nc, Nt)}
    seen = dict(tracked=0, sensed=0, colliding=0)
    worst = 0.0
    for s in range(4):
        if greedy:
            eng.step_greedy(auto_reset=0)
        else:
            eng.step_random(auto_reset=0, want_masks=True)
        assert _stepped(eng, model).all()
        worst = max(worst, _check(eng, model, (scenario, s)))
        for c, frames in S.straddling_frames(eng.unpack_masks()['camera_target_view_mask']).items():
            straddling[c] += frames
        seen['tracked'] += int(np.nansum(model.target[..., 7])); seen['sensed'] += int(model.camera[..., 1].sum()); seen['colliding'] += int(model.target[..., 8].sum())
    print(f'{scenario}: worst distance error {worst:.3e}, {seen}, frames per straddling row {straddling}')
    if Nc and eng.num_envs >= 16:      # (a single environment may see nobody in four steps)
        assert seen['tracked'] > 0 and seen['sensed'] > 0, seen
    if straddling:      # the rows the reference read did have seen targets on both sides of their word boundary
        assert sum(straddling.values()) >= 1, straddling
    # the on-demand call into guarded buffers: nothing is written behind the arrays' ends (the partial last tile)
    n = eng.num_envs
    sizes = [n * max(Nc, 0) * 2, n * Nt * 9, n * 24]
    guards = [torch.full((size + 8,), -7.0, dtype=torch.float64, device=eng.device) for size in sizes]
    pointers = [ctypes.c_void_p(g.data_ptr()) if size else None for g, size in zip(guards, sizes)]
    assert eng.lib.mate_engine_info_rows(eng._h, ctypes.c_void_p(eng.masks.data_ptr()), *pointers, eng._stream()) == 0
    torch.cuda.synchronize()
    for g, size, attached in zip(guards, sizes, (eng.info_camera_rows, eng.info_target_rows, eng.info_cargo_rows)):
        assert bool((g[size:] == -7.0).all()), scenario
        if size:
            got, ref = g[:size].view(attached.shape).clone(), attached.clone()
            if got.dim() == 3 and got.shape[2] == 9:
                assert bool(got[:, :, 6].isnan().all())
                got[:, :, 6] = ref[:, :, 6]
            assert torch.equal(got, ref), scenario


# ---------------------------------------------------------------------------------------------- 3: deliveries in every launch form
FLOWS = ['step', 'step_random', 'step_greedy', 'step_versus_greedy camera', 'step_versus_greedy target', 'rollout_random', 'rollout_greedy',
         'rollout_versus_greedy camera', 'rollout_versus_greedy target']
K = 3


def _planted(shape):
    """An engine of the shape with policies, natively reset; the planted scene; its exported reset state."""
    from mate_amd.engine import Engine
    cfg = RS.config_of(shape)
    eng = Engine(cfg, LS.BATCH, seed=LS.SEED, first_env_index=LS.FIRST)
    eng.enable_policies()
    eng.reset()
    torch.cuda.synchronize()
    flat0 = eng.export_state().cpu().numpy()
    sd = eng.state_dict_from(flat0.copy())
    tables = [[eng.lut_read(e, c) for c in range(eng.num_cameras)] for e in range(LS.BATCH)]
    scene = LS.build_scenes(sd, tables, cfg, LS.SEED, 1)[0]
    return eng, scene, flat0


def _flat_of(eng, flat0, state):
    flat = flat0.copy()
    for name, value in state.items():
        off, shape = eng.export_fields[name]
        k = int(np.prod(shape)) if shape else 1
        flat[:, off:off + k] = np.asarray(value, dtype=np.float64).reshape(LS.BATCH, k)
    return torch.from_numpy(flat)


def _standing(scene):
    """Every probe's target inside its warehouse already (half way from its landing to the centre): the logistics run on frame 0 whoever acts."""
    out = {k: np.array(v, copy=True) for k, v in scene.state.items()}
    for p in scene.plan:
        if p.side < 0:
            out['tgt_x'][p.env, p.target], out['tgt_y'][p.env, p.target] = (np.asarray(p.landing) + LS.WAREHOUSES[p.warehouse]) / 2.0
    return out


@pytest.mark.parametrize('shape', ['MATE-4v8-9', 'MATE-2v4-0'])
def test_deliveries_in_every_launch_form(shape):
    """The planted warehouse scenes (kinds delivery, shared, pick, end among the seven) through every stepping flow.  Where the caller
    moves the targets the plants walk to their landings (deliveries on frames 0 and 1, individual_done 1 exactly on the planned frame);
    where device agents or the random policy move them the probes' targets stand inside their warehouses.  Per-step flows: the rows of
    every frame equal info_ref.  Fused flows (K = 3): the rows of the last frame, individual_done all NaN, environments that stopped inside the
    launch untouched; one single step behind the fused call is measured against the fused call's last-frame goals."""
    eng, scene, flat0 = _planted(shape)
    kinds = {p.kind for p in scene.plan}
    assert {'delivery', 'shared', 'pick', 'end'} <= kinds, kinds
    n, Nc, Nt, dev = LS.BATCH, eng.num_cameras, eng.num_targets, eng.device
    walk64 = torch.from_numpy(scene.actions).to(dev)
    walk32 = walk64.float()
    goal_u = torch.from_numpy(scene.goal_u).to(dev)
    no_draws = torch.zeros((n, max(Nc, 1), Nt), dtype=torch.float64, device=dev)
    zero_cam = torch.zeros((n, Nc, 2), dtype=torch.float32, device=dev)
    walking, standing = _flat_of(eng, flat0, scene.state), _flat_of(eng, flat0, _standing(scene))
    model = _attach(eng)

    def last_masks():
        return eng._rollout['masks'][K - 1]

    single = {'step': lambda: eng.step(zero_cam.double(), walk64, tape_ct=no_draws, tape_goal=goal_u, auto_reset=False),
              'step_random': lambda: eng.step_random(auto_reset=0, want_masks=True),
              'step_greedy': lambda: eng.step_greedy(auto_reset=0),
              'step_versus_greedy camera': lambda: eng.step_versus_greedy('camera', zero_cam, auto_reset=0),
              'step_versus_greedy target': lambda: eng.step_versus_greedy('target', walk32, auto_reset=0)}
    fused = {'rollout_random': (lambda: eng.rollout_random(K, auto_reset=0, want_masks=True), 'step_random'),
             'rollout_greedy': (lambda: eng.rollout_greedy(K, auto_reset=0, want_masks=True), 'step_greedy'),
             'rollout_versus_greedy camera': (lambda: eng.rollout_versus_greedy('camera', zero_cam, K, auto_reset=0, want_masks=True), 'step_versus_greedy camera'),
             'rollout_versus_greedy target': (lambda: eng.rollout_versus_greedy('target', walk32, K, auto_reset=0, want_masks=True), 'step_versus_greedy target')}
    for flow in FLOWS:
        walks = flow in ('step', 'step_versus_greedy target', 'rollout_versus_greedy target')
        eng.import_state(walking if walks else standing)
        eng.observe()
        torch.cuda.synchronize()
        model.snapshot(eng.state_dict())                     # (the snapshot-only launch behind the import)
        planted_goals = model.goals.copy()
        delivered = 0
        if flow in single:
            live = np.ones(n, dtype=bool)
            for f in range(K):
                single[flow]()
                ran = _stepped(eng, model)
                _check(eng, model, (shape, flow, f), live & ran)
                dones = model.target[..., 6]
                delivered += int(dones[live].sum())
                if flow == 'step':
                    for p in scene.plan:
                        if p.expect == 'deliver' and p.side < 0 and live[p.env]:
                            assert dones[p.env, p.target] == (1.0 if p.frame == f else 0.0), (shape, flow, f, LS.describe([p]))
                live &= eng.scalars[:, 2].cpu().numpy() == 0      # (what a step does to an ended episode under auto_reset = 0 is no part of the contract)
        else:
            launch, then = fused[flow]
            before = [t.clone() for t in (eng.info_target_rows, eng.info_cargo_rows)]
            _, _, scalars = launch()
            ran = _stepped(eng, model, frames=K, masks=last_masks(), scalars=scalars[K - 1])
            assert ran.any()
            _check(eng, model, (shape, flow, 'last frame'))
            torch.cuda.synchronize()
            assert bool(eng.info_target_rows[:, :, 6][torch.from_numpy(ran).to(dev)].isnan().all())
            idle = torch.from_numpy(~ran).to(dev)
            for now, was in zip((eng.info_target_rows, eng.info_cargo_rows), before):
                assert torch.equal(now[idle].view(torch.int64), was[idle].view(torch.int64)), (shape, flow, 'rows of environments that stopped inside the launch')
            delivered = int(((model.goals != planted_goals) & (planted_goals >= 0))[ran].sum())
            single[then]()                                   # one single step: against the fused call's last-frame goals
            again = _stepped(eng, model)
            _check(eng, model, (shape, flow, 'single step behind'), ran & again)
            assert not np.isnan(model.target[ran & again][..., 6]).any()
        print(f'{shape} {flow}: {delivered} deliveries')
        assert delivered >= 1, (shape, flow)


# ---------------------------------------------------------------------------------------------- 4: episode boundaries
def _short(n, seed, config='MATE-4v2-9.yaml', policies=False):
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    eng = Engine(read_config(config, max_episode_steps=CUT), n, seed=seed)
    if policies:
        eng.enable_policies()
    eng.reset()
    return eng


def _equal_rows(a, b, where):
    torch.cuda.synchronize()
    for name in ('info_camera_rows', 'info_target_rows', 'info_cargo_rows'):
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x.view(torch.int64), y.view(torch.int64)), (where, name)


def test_terminal_step_and_restart_against_a_twin():
    """auto_reset = 1: at the `done` step the rows are those of a twin stepped with auto_reset = 0, bit for bit (the launch runs ahead of
    the restart), and the first step of the new episode reports individual_done 0 everywhere (the snapshot behind the restart is the new
    episode's; the twin takes an explicit masked reset)."""
    a, b = _short(40, 23), _short(40, 23)
    for eng in (a, b):
        eng.enable_info_rows()
    finished, restarted = 0, None
    for s in range(16):
        a.step_random(auto_reset=1, want_masks=True)
        b.step_random(auto_reset=0, want_masks=True)
        assert torch.equal(a.scalars, b.scalars), s
        _equal_rows(a, b, s)
        if restarted is not None:
            assert float(a.info_target_rows[restarted][:, :, 6].abs().sum()) == 0.0, s
        done = b.scalars[:, 2] > 0
        restarted = done if bool(done.any()) else None
        if restarted is not None:
            finished += int(done.sum())
            assert not torch.equal(a.export_state(), b.export_state())      # `a` has restarted: its records are the new episode's
            b.reset(env_mask=done)
            assert torch.equal(a.export_state(), b.export_state()), s
    assert finished >= 80         # every environment ended (the time limit) twice


def test_idle_environments_keep_their_terminal_rows():
    """auto_reset = 3: an environment that waits for the batched restart (done == 2) keeps the rows of its terminal step, bit for bit."""
    eng = _short(24, 29)
    eng.enable_info_rows()
    idled, kept = 0, None
    for s in range(12):
        eng.step_random(auto_reset=3, want_masks=True)
        torch.cuda.synchronize()
        now = [t.clone() for t in (eng.info_camera_rows, eng.info_target_rows, eng.info_cargo_rows)]
        idle = eng.scalars[:, 2] == 2
        if bool(idle.any()):
            idled += int(idle.sum())
            for x, y in zip(now, kept):
                assert torch.equal(x[idle].view(torch.int64), y[idle].view(torch.int64)), s
        kept = now
    assert idled > 0


@pytest.mark.parametrize('how', ['reset', 'masked reset', 'import_state'])
def test_new_records_report_no_delivery(how):
    """Behind reset(), a masked reset and import_state the snapshot-only launch runs: the next step compares with the NEW goals.  The
    imported state keeps the episode numbers and rotates every goal, so that a stale snapshot would report a delivery per loaded target."""
    eng = _short(20, 31, 'MATE-4v8-9.yaml')
    model = _attach(eng)
    Nt = eng.num_targets
    for s in range(2):
        eng.step_random(auto_reset=0, want_masks=True)
        _stepped(eng, model)
    mask = None
    if how == 'reset':
        eng.reset()
    elif how == 'masked reset':
        mask = torch.arange(20, device=eng.device) % 3 == 0
        eng.reset(env_mask=mask)
    else:
        flat = eng.export_state().cpu().numpy()
        (g_off, _), (b_off, _) = eng.export_fields['tgt_goals'], eng.export_fields['tgt_goal_bits']
        goals, bits = flat[:, g_off:g_off + Nt], flat[:, b_off:b_off + 4 * Nt].reshape(-1, Nt, 4)
        loaded = goals >= 0
        assert loaded.any()
        flat[:, g_off:g_off + Nt] = np.where(loaded, (goals + 1) % 4, goals)
        flat[:, b_off:b_off + 4 * Nt] = np.roll(bits, 1, axis=2).reshape(-1, 4 * Nt)
        eng.import_state(torch.from_numpy(flat))
        assert ((eng.state_dict()['tgt_goals'] != model.goals) & (model.goals >= 0)).any()
    torch.cuda.synchronize()
    model.snapshot(eng.state_dict(), None if mask is None else mask.cpu().numpy())
    eng.step_random(auto_reset=0, want_masks=True)
    _stepped(eng, model)
    _check(eng, model, how)
    fresh = slice(None) if mask is None else mask.cpu().numpy()
    assert float(np.abs(_rows(eng)[1][fresh][..., 6]).sum()) == 0.0


# ---------------------------------------------------------------------------------------------- 5: graph replay
def test_graph_replay_leaves_the_rows_of_direct_calls():
    """A Stepper (versus = 'camera', four steps per graph, immediate restarts) built after enabling captures the launch: after the
    warm-up and two replays the rows are those of a twin stepped directly, bit for bit, across episode ends."""
    a, b = _short(40, 37, policies=True), _short(40, 37, policies=True)
    for eng in (a, b):
        eng.enable_info_rows()
    cam = torch.linspace(-1.0, 1.0, 40 * a.num_cameras * 2, device='cuda').reshape(40, a.num_cameras, 2).contiguous()
    stepper = a.make_stepper(cam, None, auto_reset=1, graph_steps=4, versus='camera')
    ended = 0
    for _ in range(stepper.warmup_steps):
        b.step_versus_greedy('camera', cam, auto_reset=1)
    for _ in range(2):
        stepper.run(4)
        for _ in range(4):
            b.step_versus_greedy('camera', cam, auto_reset=1)
            ended += int((b.scalars[:, 2] == 1).sum())
        _equal_rows(a, b, 'replay')
        assert torch.equal(a.scalars, b.scalars)
    assert ended >= 40
    stepper.close()


# ---------------------------------------------------------------------------------------------- 6: the on-demand call
def test_on_demand_call():
    """Engine.info_rows(masks) equals the attached rows of the step just taken but for individual_done, which reads NaN; without masks the
    three mask-derived columns read NaN too and everything else stays."""
    eng = _short(17, 41, 'MATE-4v8-9.yaml')
    eng.enable_info_rows()
    eng.step_random(auto_reset=0, want_masks=True)
    attached = [t.clone() for t in (eng.info_camera_rows, eng.info_target_rows, eng.info_cargo_rows)]
    camera, target, cargo = eng.info_rows(masks=eng.masks)
    assert camera is not eng.info_camera_rows and target is not eng.info_target_rows
    assert torch.equal(camera, attached[0]) and torch.equal(cargo, attached[2])
    state_columns = [0, 1, 2, 3, 4, 5, 7, 8]
    assert torch.equal(target[:, :, state_columns], attached[1][:, :, state_columns]) and bool(target[:, :, 6].isnan().all())
    camera, target, cargo = eng.info_rows()
    assert bool(camera.isnan().all()) and bool(target[:, :, [6, 7]].isnan().all()) and torch.equal(cargo, attached[2])
    assert torch.equal(target[:, :, [0, 1, 2, 3, 4, 5, 8]], attached[1][:, :, [0, 1, 2, 3, 4, 5, 8]])
    for now, was in zip((eng.info_camera_rows, eng.info_target_rows, eng.info_cargo_rows), attached):      # the attached rows and the snapshot stay
        assert torch.equal(now, was)
    eng.step_random(auto_reset=0, want_masks=True)
    assert not bool(eng.info_target_rows[:, :, 6].isnan().any())
    plain = _short(5, 42)                  # nothing attached
    camera, target, cargo = plain.info_rows()
    assert camera.shape == (5, 4, 2) and target.shape == (5, 2, 9) and cargo.shape == (5, 24) and plain.info_target_rows is None


# ---------------------------------------------------------------------------------------------- 7: nothing else moves
def test_attaching_changes_no_other_output():
    """Observations, scalars, masks and the exported state of eight steps with restarts are bit-identical with and without the rows."""
    plain, attached = _short(33, 43, 'MATE-4v8-9.yaml'), _short(33, 43, 'MATE-4v8-9.yaml')
    attached.enable_info_rows()
    for s in range(8):
        for eng in (plain, attached):
            eng.step_random(auto_reset=1, want_masks=True)
        for name in ('camera_obs', 'target_obs', 'scalars', 'masks'):
            assert torch.equal(getattr(plain, name), getattr(attached, name)), (s, name)
        assert torch.equal(plain.export_state(), attached.export_state()), s
    assert int(plain.state_dict()['episode'].max()) >= 2      # restarts happened
    attached.disable_info_rows()
    assert attached.info_target_rows is None
    attached.step_random(auto_reset=1, want_masks=False)      # detached: the masks are optional again


# ---------------------------------------------------------------------------------------------- 8: refusals
def test_refusals_leave_the_engine_usable():
    from mate_amd._native import EngineError
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    eng = Engine(read_config('MATE-4v2-9.yaml', max_episode_steps=CUT), 8, seed=47)
    with pytest.raises(EngineError, match='before reset') as err:
        eng.enable_info_rows()
    assert err.value.code == MATE_ESTATE and eng.info_target_rows is None
    eng.enable_policies()
    eng.reset()
    rows = torch.zeros(8 * 4 * 9 + 8, dtype=torch.float64, device='cuda')
    assert eng.lib.mate_engine_enable_info_rows(eng._h, None, ctypes.c_void_p(rows.data_ptr() + 8), None) == MATE_EINVAL      # misaligned
    assert '16-byte aligned' in eng.lib.mate_engine_last_error().decode()
    assert eng.lib.mate_engine_info_rows(eng._h, None, None, ctypes.c_void_p(rows.data_ptr() + 8), None, eng._stream()) == MATE_EINVAL
    model = _attach(eng)
    before = eng.export_state().clone()
    with pytest.raises(EngineError, match='mate_engine_enable_info_rows') as err:
        eng.step_random(auto_reset=1, want_masks=False)
    assert err.value.code == MATE_EINVAL
    io = eng._io()[0]
    io.scalars_dev = None
    assert eng.lib.mate_engine_step_random(eng._h, ctypes.byref(io), 1, eng._stream()) == MATE_EINVAL
    with pytest.raises(EngineError, match='training-information rows are attached') as err:
        eng.rollout_greedy(4, auto_reset='pipelined', want_masks=True)
    assert err.value.code == MATE_ESTATE
    assert torch.equal(before, eng.export_state())            # nothing ran
    eng.step_random(auto_reset=0, want_masks=True)
    _stepped(eng, model)
    _check(eng, model, 'behind the refusals')
    # detach, step, re-attach: correct from the next step
    eng.disable_info_rows()
    eng.step_random(auto_reset=0, want_masks=False)
    model = _attach(eng)
    eng.step_random(auto_reset=0, want_masks=True)
    _stepped(eng, model)
    _check(eng, model, 're-attached')
    nav = Engine(read_config('MATE-Navigation.yaml'), 4, seed=48)
    nav.reset()
    buf = torch.zeros(64, dtype=torch.float64, device='cuda')
    assert nav.lib.mate_engine_enable_info_rows(nav._h, ctypes.c_void_p(buf.data_ptr()), None, None) == MATE_EINVAL
    assert 'no cameras' in nav.lib.mate_engine_last_error().decode()
    camera, target, cargo = nav.enable_info_rows()            # (`camera` is silently off without cameras)
    assert camera is None and nav.info_camera_rows is None and target.shape == (4, nav.num_targets, 9)
    nav.step_random(auto_reset=0, want_masks=True)
    assert set(nav.info()) == {'goal', 'goal_distance', 'warehouse_distances', 'individual_done', 'is_tracked', 'is_colliding',
                               'remaining_cargo_counts', 'awaiting_cargo_counts', 'remaining_cargoes'}


# ---------------------------------------------------------------------------------------------- 9: the batched environment
def test_batched_environment_training_information():
    from mate_amd.environment import BatchedMultiAgentTracking
    N = 20
    env = BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=N, seed=4, training_information=True, max_episode_steps=CUT)
    env.reset()
    rows = env.engine.info_target_rows
    shapes = {'num_tracked': (N, 4), 'is_sensed': (N, 4), 'goal': (N, 8), 'goal_distance': (N, 8), 'warehouse_distances': (N, 8, 4), 'individual_done': (N, 8),
              'is_tracked': (N, 8), 'is_colliding': (N, 8), 'remaining_cargo_counts': (N, 4), 'awaiting_cargo_counts': (N, 4), 'remaining_cargoes': (N, 4, 4),
              'coverage_rate': (N,), 'real_coverage_rate': (N,), 'mean_transport_rate': (N,), 'num_delivered_cargoes': (N,), 'normalized_raw_reward': (N,)}
    for s in range(9):
        env.step_random()
        infos = env.infos()
        assert {k: tuple(v.shape) for k, v in infos.items()} == shapes
        assert env.engine.info_target_rows is rows          # the same tensors at every call
        dones = env.target_dones()
        assert dones.dtype == torch.bool and dones.shape == (N, 8) and torch.equal(dones, rows[:, :, 6] == 1.0)
        assert torch.equal(infos['goal'], rows[:, :, 0]) and torch.equal(infos['remaining_cargoes'].reshape(N, 16), env.engine.info_cargo_rows[:, 8:])
        assert torch.equal(infos['coverage_rate'], env.engine.scalars[:, 3])
    _, _, done, info = env.rollout_random(3)
    infos = env.infos()
    assert bool(infos['individual_done'][~info['skipped'][-1]].isnan().all()) and torch.equal(infos['coverage_rate'], info['coverage_rate'][-1])
    with pytest.raises(RuntimeError, match='3 frames'):
        env.target_dones()
    env.step_random()
    assert not bool(env.infos()['individual_done'].isnan().any())
    plain = BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=4, seed=4)
    plain.reset()
    with pytest.raises(AssertionError, match='training_information'):
        plain.infos()
