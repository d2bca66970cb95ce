"""GPU tests of the Naive and Random opponents and the per-episode opponent mixtures (mate_engine_set_opponent_mixture, csrc/scripted_rows.hpp):
scripted_opponent_kernel on Philox draws against the NumPy restatement of tests/scripted_ref.py, read back through the launch's record; the mixture
draw's frequencies; the external rows; batched restarts and graph replay against direct calls; idle environments; single-candidate mixtures against the
plain selections; the refusals."""
import numpy as np
import pytest
import torch

import gpu_util as U
import scripted_ref as R

pytestmark = pytest.mark.gpu

ESTATE, EINVAL = -4, -1
ONE_LAUNCH_FLOWS = (3, 4)      # FLOW_GREEDY / FLOW_STEP_GREEDY (csrc/engine_kernels.hpp): the agents and the step in one kernel
ALL_FOUR = {'greedy': 1.0, 'heuristic': 1.0, 'naive': 2.0, 'random': 1.0}
NO_HEURISTIC = {'greedy': 1.0, 'naive': 2.0, 'random': 1.0}


def _engine(config, n, kw=None, seed=23, **more):
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    cfg = read_config(config, **(kw or {})) if isinstance(config, str) else config
    eng = Engine(cfg, n, seed=seed, **more)
    eng.enable_policies()
    eng.reset()
    return eng, cfg


def _plant_emptied_warehouses(eng):
    """Every third environment, as tests/logistics_scenes.py plants its scenes (import_state): warehouses 1 and 2 hold nothing and every target knows it;
    every other target carries nothing, and all of them stand inside the four warehouses in turn -- a Naive target whose first goal is the warehouse
    it stands in arrives at once: with its cargo in the one-increment form, with none (and not every warehouse empty) in the skip-empties form, over
    one or two warehouses by its direction."""
    sd = eng.state_dict()
    Nt = eng.num_targets
    planted = np.arange(eng.num_envs) % 3 == 0
    f = {k: np.array(sd[k], dtype=np.float64, copy=True) for k in ('tgt_x', 'tgt_y', 'tgt_goals', 'tgt_goal_bits', 'tgt_empty_bits', 'freights', 'bounties',
                                                                    'remaining_cargoes', 'awaiting_cargo_counts')}
    rng = np.random.RandomState(3)
    for e in np.flatnonzero(planted):
        f['remaining_cargoes'][e, 1:3] = 0
        f['tgt_empty_bits'][e][:, 1:3] = 1
        for key in ('tgt_goals', 'tgt_goal_bits', 'freights', 'bounties'):      # every other target keeps the cargo it started with
            f[key][e, ::2] = -1 if key == 'tgt_goals' else 0
        for t in range(Nt):
            w = (t + e) % 4
            f['tgt_x'][e, t] = R.WAREHOUSES[w, 0] + rng.uniform(-30.0, 30.0)
            f['tgt_y'][e, t] = R.WAREHOUSES[w, 1] + rng.uniform(-30.0, 30.0)
        f['awaiting_cargo_counts'][e] = f['remaining_cargoes'][e].sum(axis=0) + f['tgt_goal_bits'][e].sum(axis=0)
    eng.load_state_dict(f)
    eng.observe()
    return planted


def _kinds(mixture):
    return [R.SCRIPTED_AGENTS.index(name) for name in mixture]


@pytest.mark.parametrize('config,n,steps,kw,flow,cam_mix,tgt_mix', [
    ('MATE-4v8-9.yaml', 96, 150, {'max_episode_steps': 60}, 'versus', None, ALL_FOUR),      # immediate restarts fall inside the run
    ('MATE-4v8-9.yaml', 96, 150, {'max_episode_steps': 60}, 'selected', None, ALL_FOUR),
    ('MATE-4v8-9.yaml', 96, 60, {'max_episode_steps': 20}, 'greedy', ALL_FOUR, ALL_FOUR),   # both teams, the Heuristic cameras among the candidates
    ('MATE-8v8-9.yaml', 65, 40, {'max_episode_steps': 12}, 'greedy', NO_HEURISTIC, ALL_FOUR),      # a partial tile: 16 environments per workgroup plus one
    ('MATE-2v4-0.yaml', 33, 60, {'max_episode_steps': 20}, 'greedy', ALL_FOUR, ALL_FOUR),          # no obstacles, sub-wave shape
    ('MATE-Navigation.yaml', 17, 40, {'max_episode_steps': 12}, 'greedy', NO_HEURISTIC, ALL_FOUR), # no cameras: the camera mixture is installed and never plays
    ('7v5-3', None, 40, {}, 'greedy', NO_HEURISTIC, ALL_FOUR),                              # tests/shape_edges.py ATTACHED_CASES (n, seed, first_env_index are the case's)
    ('16v16-9', None, 40, {}, 'greedy', NO_HEURISTIC, ALL_FOUR),                            # every lane of a group is a camera and a target
    ('0v5-64', None, 40, {}, 'greedy', NO_HEURISTIC, ALL_FOUR),
])
def test_scripted_batch_against_the_restatement(config, n, steps, kw, flow, cam_mix, tgt_mix):
    """On Philox draws: the state is read before every step, the record, the source rows and the final rows after it.  Every final row equals the
    restatement's to 1e-9 wherever no branch condition lies within 1e-9 (relative) of equality (at most 0.1 % of the entries may), bit for bit where no
    arithmetic of the device's went into it; the record is finite exactly where the restatement used a draw; every candidate is chosen in some episode."""
    import shape_edges
    from mate_amd.config import read_config, scenario_tables
    from mate_amd.engine import Engine
    shipped = config.endswith('.yaml')
    if shipped:
        cfg, seeds = read_config(config, **kw), dict(seed=23)
    else:
        case = shape_edges.attached_case(config)
        cfg, n, seeds = dict(shape_edges.case_scenario(case), max_episode_steps=12), case.n, dict(seed=case.seed, first_env_index=case.first)
    eng = Engine(cfg, n, **seeds)
    eng.enable_policies()
    eng.reset()
    Nc, Nt = eng.num_cameras, eng.num_targets
    planted = _plant_emptied_warehouses(eng) if config == 'MATE-4v8-9.yaml' else None
    if cam_mix is not None:
        eng.set_opponent_mixture('camera', cam_mix, random_frame_skip=5)
    eng.set_opponent_mixture('target', tgt_mix, random_frame_skip=7)
    record = eng.scripted_record()
    eng.scripted_tape(record=record)
    cam = scenario_tables(cfg)['camera']
    teams = {}
    if cam_mix is not None and Nc > 0 and flow == 'greedy':
        teams[0] = R.ScriptedTeam(0, n, Nc, frame_skip=5)
    teams[1] = R.ScriptedTeam(1, n, Nt, frame_skip=7)
    gen = torch.Generator(device='cpu').manual_seed(5)
    mine = torch.zeros((n, max(Nc, 1), 2), device=eng.device)
    if flow == 'selected':
        eng.enable_selection(multi_selection=True)
    chosen = {team: set() for team in teams}
    entries = skipped = once = skip = far = resampled = kept = 0
    worst = 0.0
    for s in range(steps):
        sd = eng.state_dict()
        if flow == 'versus':
            mine.copy_((torch.rand(mine.shape, generator=gen) * 2.0 - 1.0) * 3.0)
            eng.step_versus_greedy('camera', mine)
        elif flow == 'selected':
            eng.step_selected()
        else:
            eng.step_greedy()
        assert eng.last_flow not in ONE_LAUNCH_FLOWS
        finals = [a.cpu().numpy() for a in eng.policy_actions()]
        rec = {k: v.cpu().numpy() for k, v in record.items()}
        live = np.ones(n, dtype=bool)
        for team, ref in teams.items():
            mixture = cam_mix if team == 0 else tgt_mix
            rows = {R.SCRIPTED_AGENTS.index(name): eng.scripted_rows(team, name).cpu().numpy() for name in mixture if name in ('greedy', 'heuristic')}
            if team == 0:
                high = np.broadcast_to(np.array([cam['rotation_step'], cam['zooming_step']]), (n, Nc, 2))
                draws, targets = dict(u=rec['camera_u']), None
            else:
                step_size = cfg['target']['step_size'] / sd['tgt_capacity']
                high = np.stack([step_size, step_size], axis=-1)
                draws = dict(u=rec['target_u'], reset=rec['target_reset'])
                empty = (sd['tgt_empty_bits'].reshape(n, Nt, 4) != 0).astype(np.int64) @ np.array([1, 2, 4, 8])
                targets = dict(xy=np.stack([sd['tgt_x'], sd['tgt_y']], axis=-1), carries=(sd['tgt_goal_bits'].reshape(n, Nt, 4) != 0).any(-1), empty_bits=empty)
            choice = rec['choice'][team]
            assert np.isin(choice, _kinds(mixture)).all()
            out = ref.step(live, sd['episode'].astype(np.int64), choice, rows, high, draws, targets)
            chosen[team] |= set(choice.tolist())
            got = finals[team]
            assert np.array_equal(np.isfinite(draws['u']), out['used_u']), (s, team)
            if team == 1:
                assert np.array_equal(np.isfinite(draws['reset']), out['used_reset']), s
            exact = np.broadcast_to(out['exact'][..., None], got.shape)
            assert np.array_equal(got[exact], out['final'][exact]), (s, team)
            near = out['margin'] < 1e-9
            diff = np.abs(got - out['final']).max(-1)
            entries += diff.size; skipped += int(near.sum())
            if (~near).any():
                worst = max(worst, float(diff[~near].max()))
            assert worst < 1e-9, (s, team, worst)
            wrong = near & (diff >= 1e-9)
            if wrong.any():      # the restatement took the other side of a rim: follow the engine from here (the memory is the engine's to define)
                mem = eng.scripted_memory(team)
                ref.naive['goal'][wrong] = mem['goal'].cpu().numpy()[wrong]
                ref.naive['prev_noise'][wrong] = mem['prev_noise'].cpu().numpy()[wrong]
            if team == 1 and out['info'] is not None and config == 'MATE-4v8-9.yaml':
                info = out['info']
                once += int(info['once'].sum()); skip += int(info['skip'].sum()); far += int((info['skip'] & (info['skipped'] >= 2)).sum())      # over more than one warehouse, as the restatement's census counts it
                resampled += int(info['resample'].sum()); kept += int((~info['resample'] & ~np.broadcast_to(out['exact'], info['resample'].shape)).sum())
        if s == steps - 1:       # the memory the launch keeps is the restatement's
            for team, ref in teams.items():
                mem = {k: v.cpu().numpy() for k, v in eng.scripted_memory(team).items()}
                assert np.array_equal(mem['choice'], ref.choice) and np.array_equal(mem['counter'], ref.counter)
                was_random = np.isin(R.RANDOM, list(chosen[team]))
                assert not was_random or np.array_equal(mem['prev_action'][ref.choice == R.RANDOM], ref.prev_action[ref.choice == R.RANDOM])
    print(config, flow, steps, 'steps:', entries, 'entries,', skipped, 'near a rim, worst', worst, 'arrivals', once, skip, far, 'noise', resampled, kept)
    assert skipped <= 1e-3 * entries
    for team in teams:
        mixture = cam_mix if team == 0 else tgt_mix
        assert chosen[team] == set(_kinds(mixture)), (team, chosen[team])
    if planted is not None:
        assert once > 0 and skip > 0 and far > 0 and resampled > 0 and kept > 0, (once, skip, far, resampled, kept)


def test_mixture_frequencies_and_the_hold():
    """4096 x 2 environments, weights [1, 3]: the first draw's frequencies lie within 4 standard errors of 1/4 and 3/4, on both teams, independently."""
    n = 8192
    eng, cfg = _engine('MATE-4v8-9.yaml', n, seed=77)
    eng.set_opponent_mixture('target', ['naive', 'random'], [1.0, 3.0])
    eng.set_opponent_mixture('camera', {'random': 1.0, 'greedy': 0.0, 'naive': 3.0})      # (a zero weight: never drawn, not in the cumulative table)
    eng.step_greedy()
    se = np.sqrt(0.25 * 0.75 / n)
    tgt = eng.scripted_memory('target')['choice'].cpu().numpy()
    cam = eng.scripted_memory('camera')['choice'].cpu().numpy()
    assert set(tgt.tolist()) == {R.NAIVE, R.RANDOM} and set(cam.tolist()) == {R.NAIVE, R.RANDOM}
    assert abs((tgt == R.NAIVE).mean() - 0.25) < 4 * se and abs((cam == R.RANDOM).mean() - 0.25) < 4 * se, ((tgt == R.NAIVE).mean(), (cam == R.RANDOM).mean())
    both = ((tgt == R.NAIVE) & (cam == R.RANDOM)).mean()
    assert abs(both - 0.0625) < 4 * np.sqrt(0.0625 * 0.9375 / n), both      # the teams draw on words of their own
    eng.step_greedy()
    assert np.array_equal(eng.scripted_memory('target')['choice'].cpu().numpy(), tgt)


def test_mixture_frequencies_with_four_unequal_weights():
    """The cumulative table beyond two candidates: 8192 environments, weights 1 : 2 : 5 : 2 in an order that is not the kinds' -- every candidate's
    frequency lies within 4 standard errors (sqrt(p (1 - p) / n)) of its weight."""
    n = 8192
    eng, cfg = _engine('MATE-4v8-9.yaml', n, seed=78)
    order, weights = ['random', 'greedy', 'naive', 'external'], np.array([1.0, 2.0, 5.0, 2.0])
    eng.set_opponent_mixture('target', order, weights.tolist())
    eng.step_versus_greedy('camera', torch.zeros((n, eng.num_cameras, 2), device=eng.device))
    choice = eng.scripted_memory('target')['choice'].cpu().numpy()
    for name, p in zip(order, weights / weights.sum()):
        freq = (choice == R.SCRIPTED_AGENTS.index(name)).mean()
        assert abs(freq - p) < 4 * np.sqrt(p * (1 - p) / n), (name, freq, p)


def test_greedy_agents_that_sat_out_reset_when_a_changed_mixture_brings_them_back():
    """{naive} -> {greedy, naive} inside one episode: both mixtures launch, the Greedy targets sat out under the first.  Their row at the first call
    under the second is that of Greedy agents that run their reset on that state -- a second engine given the first one's state, whose Greedy targets
    have never acted -- not one computed from the location and noise they remembered."""
    from mate_amd.engine import Engine
    n = 32
    eng, cfg = _engine('MATE-4v8-9.yaml', n, seed=31)
    mine = torch.zeros((n, eng.num_cameras, 2), device=eng.device)
    for _ in range(3):
        eng.step_versus_greedy('camera', mine, auto_reset=False)      # the Greedy targets act: their tag is this episode's
    eng.set_opponent_mixture('target', 'naive')
    for _ in range(6):
        eng.step_versus_greedy('camera', mine, auto_reset=False)      # ... and sit out while the Naive targets walk
    eng.set_opponent_mixture('target', ['greedy', 'naive'])
    twin = Engine(cfg, n, seed=31)
    twin.enable_policies()
    twin.import_state(eng.export_state())
    eng.step_versus_greedy('camera', mine, auto_reset=False)
    twin.step_versus_greedy('camera', mine, auto_reset=False)
    assert torch.equal(eng.scripted_rows('target', 'greedy'), twin.policy_actions()[1])


def test_external_rows_and_taped_draws():
    """Rows the caller wrote arrive in exactly the environments that drew 'external'; a second engine fed the first one's record as its tape plays the same bytes."""
    n = 48
    first, cfg = _engine('MATE-4v8-9.yaml', n, {'max_episode_steps': 10})
    second, _ = _engine('MATE-4v8-9.yaml', n, {'max_episode_steps': 10})
    mixture = {'external': 1.0, 'naive': 1.0, 'greedy': 1.0, 'random': 1.0}
    records = []
    for eng in (first, second):
        eng.set_opponent_mixture('target', mixture, random_frame_skip=3)
        eng.set_opponent_mixture('camera', {'external': 1.0, 'naive': 1.0, 'random': 2.0}, random_frame_skip=4)
        records.append(eng.scripted_record())
    first.scripted_tape(record=records[0])
    gen = torch.Generator(device='cpu').manual_seed(11)
    seen = set()
    for s in range(25):
        rows = [(torch.rand((n, k, 2), generator=gen, dtype=torch.float64) - 0.5).to(first.device) for k in (first.num_cameras, first.num_targets)]
        for eng in (first, second):
            eng.external_actions('camera').copy_(rows[0]); eng.external_actions('target').copy_(rows[1])
        first.step_greedy()
        tape = {k: torch.nan_to_num(v, nan=0.25) if v.dtype == torch.float64 else v.clone() for k, v in records[0].items()}
        second.scripted_tape(tape=tape, record=records[1])
        second.step_greedy()
        choice = records[0]['choice'].cpu().numpy()
        for team, final in enumerate(first.policy_actions()):
            ext = torch.from_numpy(choice[team] == R.EXTERNAL).to(first.device)
            assert torch.equal(final[ext], rows[team][ext]) and not (final[~ext] == rows[team][~ext]).all(-1).all(-1).any(), s
            seen |= {(team, int(k)) for k in choice[team]}
        for a, b in zip(first.policy_actions(), second.policy_actions()):
            assert torch.equal(a, b), s
        assert torch.equal(first.export_state(), second.export_state()), s
        for k in records[0]:
            assert torch.equal(torch.nan_to_num(records[0][k].double(), nan=-7.0), torch.nan_to_num(records[1][k].double(), nan=-7.0)), (s, k)
    assert (0, R.EXTERNAL) in seen and (1, R.EXTERNAL) in seen and len(seen) == 7


def test_batched_restarts_idle_environments_and_graph_replay():
    """auto_reset = 4 over episodes of 25 steps: an environment that idles (done = 2) until the interval's restart keeps memory, choice and final row; the graph
    stepper's replay of whole intervals (make_stepper(versus='camera', graph_steps=8)) equals the direct calls bit for bit."""
    n, k = 64, 4
    direct, cfg = _engine('MATE-4v8-9.yaml', n, {'max_episode_steps': 25}, seed=9)
    graphed, _ = _engine('MATE-4v8-9.yaml', n, {'max_episode_steps': 25}, seed=9)
    for eng in (direct, graphed):
        eng.set_opponent_mixture('target', ALL_FOUR, random_frame_skip=6)
    mine = [torch.zeros((n, eng.num_cameras, 2), device=eng.device) for eng in (direct, graphed)]
    counters = [torch.zeros((), device=direct.device) for _ in range(2)]

    def policy(i):
        def between():
            counters[i].add_(1.0)
            mine[i].copy_((torch.sin(counters[i]) * 4.0).expand_as(mine[i]))
        return between

    stepper = graphed.make_stepper(mine[1], None, auto_reset=k, graph_steps=2 * k, between=policy(1), versus='camera')
    assert stepper.graph is not None
    total = stepper.warmup_steps + 5 * 2 * k
    idle_rows = 0
    before = None
    for s in range(total):
        policy(0)()
        direct.step_versus_greedy('camera', mine[0], auto_reset=k)
        now = dict(direct.scripted_memory('target'), final=direct.policy_actions()[1])
        idle = direct.scalars[:, 2] == 2      # no step ran in this call: the agents' launch skipped the environment
        if before is not None and bool(idle.any()):
            for key in now:
                assert torch.equal(now[key][idle], before[key][idle]), (s, key)
            idle_rows += int(idle.sum())
        before = now
    assert idle_rows > 0
    for _ in range(5):
        stepper.run(2 * k)
    for a, b in ((direct.scalars, graphed.scalars), (direct.masks, graphed.masks), (direct.camera_obs, graphed.camera_obs), (direct.target_obs, graphed.target_obs),
                 (direct.export_state(), graphed.export_state())):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for a, b in zip(direct.policy_actions(), graphed.policy_actions()):
        assert torch.equal(a, b)
    for key, value in direct.scripted_memory('target').items():
        assert torch.equal(value, graphed.scripted_memory('target')[key]), key
    stepper.close()


@pytest.mark.parametrize('name', ['greedy', 'heuristic'])
def test_single_candidate_mixture_is_the_plain_selection(name):
    """{greedy: 1} against no mixture at all, {heuristic: 1} against set_*_opponent('heuristic'): scalars, rows, masks, export_state, the launch forms."""
    n = 40
    plain, cfg = _engine('MATE-4v8-9.yaml', n, {'max_episode_steps': 15}, seed=4)
    mixed, _ = _engine('MATE-4v8-9.yaml', n, {'max_episode_steps': 15}, seed=4)
    if name == 'heuristic':
        plain.set_target_opponent('heuristic'); plain.set_camera_opponent('heuristic')
    mixed.set_opponent_mixture('target', name)
    mixed.set_opponent_mixture('camera', {name: 2.5})
    mine = torch.zeros((n, plain.num_cameras, 2), device=plain.device)
    for s in range(24):
        for eng in (plain, mixed):
            if s % 3 == 2:
                eng.step_versus_greedy('camera', mine)
            else:
                eng.step_greedy()
        assert plain.last_flow == mixed.last_flow
        for a, b in ((plain.scalars, mixed.scalars), (plain.masks, mixed.masks), (plain.camera_obs, mixed.camera_obs), (plain.target_obs, mixed.target_obs),
                     (plain.export_state(), mixed.export_state())):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), s
        for a, b in zip(plain.policy_actions(), mixed.policy_actions()):
            assert torch.equal(a, b), s
    if name == 'greedy':         # the fused launches stay available under {greedy}
        assert plain.last_flow in ONE_LAUNCH_FLOWS
        plain.rollout_greedy(4); mixed.rollout_greedy(4)
        assert torch.equal(plain.export_state(), mixed.export_state())


def test_refusals_leave_the_engine_as_it_was():
    """Every error code of mate_engine_set_opponent_mixture and of what a mixture refuses, with a message that names the mixture; export_state is unchanged
    afterwards and the engine still steps."""
    from mate_amd._native import EngineError
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    import ctypes
    cfg = read_config('MATE-4v8-9.yaml')
    n = 16
    bare = Engine(cfg, n, seed=1)

    def raw(eng, team, kinds, weights, skip=20):
        k = (ctypes.c_int32 * len(kinds))(*kinds)
        w = (ctypes.c_double * len(kinds))(*weights)
        status = eng.lib.mate_engine_set_opponent_mixture(eng._h, team, k, w, len(kinds), skip)
        return status, eng.lib.mate_engine_last_error().decode()

    status, message = raw(bare, 1, [2], [1.0])
    assert status == ESTATE and 'mixture' in message and 'policy_enable' in message
    bare.close()

    eng, _ = _engine(cfg, n, seed=1)
    state = eng.export_state().clone()
    for kinds, weights, skip in (([7], [1.0], 20), ([2, 2], [1.0, 1.0], 20), ([2, 3], [1.0, -1.0], 20), ([2, 3], [1.0, float('nan')], 20),
                                 ([2, 3], [1.0, float('inf')], 20), ([2, 3], [0.0, 0.0], 20), ([2, 3], [1.0, 1.0], 0)):
        for team in (0, 1):
            status, message = raw(eng, team, kinds, weights, skip)
            assert status == EINVAL and 'mixture' in message, (kinds, weights, skip, message)
    status, message = raw(eng, 0, [0, 1], [1.0, 1.0])                    # a Heuristic camera candidate without its tables
    assert status == ESTATE and 'mixture' in message and 'tables' in message
    odd = torch.zeros(n * eng.num_cameras * 2 + 1, dtype=torch.float64, device=eng.device)[1:]      # 8 bytes off a 16-byte boundary
    pointers = [None] * 8
    pointers[4] = ctypes.c_void_p(odd.data_ptr())
    assert eng.lib.mate_engine_scripted_tape(eng._h, *pointers) == EINVAL and '16 bytes' in eng.lib.mate_engine_last_error().decode()
    eng.set_obs_mode(target='enhanced')
    status, message = raw(eng, 1, [1, 2], [1.0, 1.0])                    # a Heuristic candidate under a non-plain mode of the team
    assert status == EINVAL and 'mixture' in message and 'mode' in message
    eng.set_obs_mode()
    assert eng.mixtures == [None, None]
    assert torch.equal(eng.export_state(), state)
    eng.step_greedy()
    assert eng.last_flow in ONE_LAUNCH_FLOWS                              # nothing was installed

    eng.set_opponent_mixture('target', ['greedy', 'naive'])
    state = eng.export_state().clone()
    with pytest.raises(EngineError) as err:
        eng.set_target_opponent('heuristic')
    assert err.value.code == ESTATE and 'mixture' in str(err.value)
    eng.set_camera_opponent('greedy')                                     # (the other team has none)
    mine = torch.zeros((n, eng.num_cameras, 2), device=eng.device)
    for call in (lambda: eng.rollout_greedy(4), lambda: eng.rollout_versus_greedy('camera', mine, 4)):
        with pytest.raises(EngineError) as err:
            call()
        assert err.value.code == ESTATE and 'mixture' in str(err.value)
    with pytest.raises(ValueError, match='mixture'):
        eng.make_stepper(mine, None, versus='camera', frame_skip=4)
    with pytest.raises(EngineError) as err:
        eng.scripted_rows('target', 'heuristic')      # no such source in this mixture
    assert err.value.code == ESTATE
    assert torch.equal(eng.export_state(), state)
    eng.rollout_versus_greedy('target', torch.zeros((n, eng.num_targets, 2), device=eng.device), 2)      # the caller plays the mixed team: unaffected
    eng.step_versus_greedy('camera', mine)
    assert eng.last_flow not in ONE_LAUNCH_FLOWS
    eng.clear_opponent_mixture('target')
    assert eng.mixtures == [None, None] and eng.target_agent == 'greedy'
    eng.set_target_opponent('heuristic'); eng.set_target_opponent('greedy')
    eng.rollout_greedy(3)
    eng.step_greedy()
    assert eng.last_flow in ONE_LAUNCH_FLOWS


def test_environment_classes_and_evaluate_run():
    """BatchedMultiAgentTracking(target_mixture=, camera_mixture=), the N = 1 class through enable_greedy_policies, and
    `python -m mate_amd.evaluate --num-envs 8 --target-mixture naive --episodes 2` (its main(), in this process)."""
    import mate_amd
    from mate_amd.evaluate import main
    env = mate_amd.BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=8, max_episode_steps=10, target_mixture={'naive': 1.0, 'random': 1.0}, camera_mixture='naive')
    assert env.engine.mixtures == [{'naive': 1.0}, {'naive': 1.0, 'random': 1.0}]
    env.reset()
    for _ in range(12):
        env.engine.step_greedy()
    assert env.engine.last_flow not in ONE_LAUNCH_FLOWS
    cam = env.engine.policy_actions()[0]
    assert bool((cam >= 0).all()) and bool((cam > 0).any())       # the Naive cameras turn anti-clockwise and zoom out
    assert set(env.engine.scripted_memory('target')['choice'].tolist()) <= {R.NAIVE, R.RANDOM}
    env.close()
    one = mate_amd.MultiAgentTracking('MATE-4v2-9.yaml', max_episode_steps=10)
    one.enable_greedy_policies(target_mixture='naive', camera_mixture={'greedy': 1.0, 'random': 1.0})
    one.reset()
    for _ in range(5):
        one.step_greedy()
    assert one.engine.scripted_memory('target')['choice'].tolist() == [R.NAIVE]
    records = main(['--config', 'MATE-4v8-9.yaml', '--num-envs', '8', '--target-mixture', 'naive', '--episodes', '2', '--max-episode-steps', '20'])
    assert records.shape == (2, 16) and np.isfinite(records[:, :14]).all()      # (column 14, num_tracked, is kept for the camera team only)


REPLAY_FIXTURES = ['naive_4v8-9', 'naive_2v4-0', 'naive_8v8-9', 'random_4v8-9', 'random_2v4-0']


@pytest.mark.parametrize('versus_camera', [False, True], ids=['step_greedy', 'versus_camera'])
@pytest.mark.parametrize('name', REPLAY_FIXTURES)
def test_closed_loop_replay_of_the_recorded_reference(name, versus_camera):
    """The reference's episode (tests/golden/make_scripted_golden.py) replayed with N = 2 and f64 observations, environment and agent draws from tapes:
    through step_greedy (both teams the recorded pair) and through step_versus_greedy with the recorded camera actions.  Joint actions and target
    positions within 1e-8; view masks, goals, bounties and episode reward equal."""
    import golden_util as G
    fx = G.load(name + '.npz')
    pair = str(fx['policy'])
    N = 2
    eng = U.engine_from_fixture(fx, N, obs_dtype=torch.float64)
    eng.enable_policies()
    eng.set_opponent_mixture('target', pair)
    if not versus_camera:
        eng.set_opponent_mixture('camera', pair)
    dev = eng.device
    tape0 = torch.from_numpy(np.where(fx['reset/camera_target_view_mask'], 1.0, 0.0)[None].repeat(N, 0)).to(dev)
    eng.observe(tape_ct=tape0)
    draws = R.fixture_draws(fx)

    def bc(a, dtype=np.float64):
        a = np.asarray(a)
        return torch.from_numpy(np.broadcast_to(a, (N,) + a.shape).astype(dtype).copy()).to(dev)

    reset = bc(np.nan_to_num(draws['target_reset'], nan=0.0))
    T = len(fx['step/done'])
    worst = {'camera': 0.0, 'target': 0.0, 'xy': 0.0}
    for s in range(T):
        eng.scripted_tape(tape=dict(camera_u=bc(np.nan_to_num(draws['camera_u'][s], nan=0.0)), target_u=bc(np.nan_to_num(draws['target_u'][s], nan=0.0)), target_reset=reset))
        env_tape = bc(np.nan_to_num(fx['step/tape_ct'][s], nan=0.0))
        goal_tape = bc(np.nan_to_num(fx['step/goal_u'][s], nan=0.0))
        if versus_camera:
            eng.step_versus_greedy('camera', bc(fx['step/cam_act'][s]), tape_ct=env_tape, tape_goal=goal_tape, auto_reset=False)
        else:
            eng.step_greedy(tape_ct=env_tape, tape_goal=goal_tape, auto_reset=False)
        assert eng.last_flow not in ONE_LAUNCH_FLOWS
        cam_act, tgt_act = (a.cpu().numpy() for a in eng.policy_actions())
        sd = eng.state_dict()
        for e in range(N):
            worst['target'] = max(worst['target'], np.abs(tgt_act[e] - fx['step/tgt_act'][s]).max())
            if not versus_camera:
                worst['camera'] = max(worst['camera'], np.abs(cam_act[e] - fx['step/cam_act'][s]).max())
            worst['xy'] = max(worst['xy'], np.abs(sd['tgt_x'][e] - fx['step/tgt_xy'][s][:, 0]).max(), np.abs(sd['tgt_y'][e] - fx['step/tgt_xy'][s][:, 1]).max())
        assert worst['camera'] < 1e-8 and worst['target'] < 1e-8 and worst['xy'] < 1e-8, (s, worst)
        masks = eng.unpack_masks()
        assert np.array_equal(masks['camera_target_view_mask'][0], fx['step/camera_target_view_mask'][s]), s
        assert np.array_equal(sd['tgt_goals'][0], fx['step/tgt_goals'][s].astype(np.float64)), s
        assert np.array_equal(sd['bounties'][1], fx['step/bounties'][s].astype(np.float64)), s
        assert sd['episode_reward'][0] == fx['step/episode_reward'][s], s
    print(name, 'versus camera' if versus_camera else 'step_greedy', T, 'steps, worst differences', worst)


def test_closed_loop_replay_of_the_recorded_mixture_across_its_restarts():
    """mixture_4v8-9.npz: the reference's MultiCamera-side view of MixtureTargetAgent([Greedy, Naive, Random], [1, 2, 1]) through the 8 episodes of one
    environment object, replayed on ONE engine with N = 2 and f64 observations: every episode starts from the state the reference's reset() left
    (import_state, the episode number advanced, so the mixture's reset and the candidate's run at the first call), `choice` and every agent and
    environment draw come from tapes, the camera actions are the recorded ones (step_versus_greedy).  Joint actions and target positions within 1e-8;
    view masks, goals, bounties and episode reward equal; the record reports the taped candidate on every frame."""
    import golden_util as G
    fx = G.load('mixture_4v8-9.npz')
    names = [str(c) for c in fx['candidates']]
    episodes = R.mixture_episodes(fx)
    N = 2
    eng = U.engine_from_fixture(episodes[0], N, obs_dtype=torch.float64)
    eng.enable_policies()
    eng.set_opponent_mixture('target', names, [float(w) for w in fx['weights']])
    dev = eng.device
    record = eng.scripted_record()

    def bc(a, dtype=np.float64):
        a = np.asarray(a)
        return torch.from_numpy(np.broadcast_to(a, (N,) + a.shape).astype(dtype).copy()).to(dev)

    worst = {'target': 0.0, 'xy': 0.0}
    played = []
    for k, ep in enumerate(episodes):
        if k:
            U.load_fixture_state(eng, ep)                # the reference's reset() behind episode k - 1
        eng.load_state_dict({'episode': np.full(N, k + 1.0)})
        eng.observe(tape_ct=torch.from_numpy(np.where(ep['reset/camera_target_view_mask'], 1.0, 0.0)[None].repeat(N, 0)).to(dev))
        m0 = eng.unpack_masks()
        assert np.array_equal(m0['camera_target_view_mask'][0], ep['reset/camera_target_view_mask'])
        assert np.array_equal(m0['target_camera_view_mask'][1], ep['reset/target_camera_view_mask'])
        kind = R.SCRIPTED_AGENTS.index(names[int(ep['choice'][0])])
        played.append(kind)
        draws = R.fixture_draws(ep)
        reset = bc(np.nan_to_num(draws['target_reset'], nan=0.0))
        choice = torch.full((2, N), -1, dtype=torch.int32, device=dev)
        for s in range(len(ep['step/done'])):
            choice[1] = kind if s == 0 else -1           # (only a team's first call of an episode reads it)
            eng.scripted_tape(tape=dict(target_u=bc(np.nan_to_num(draws['target_u'][s], nan=0.0)), target_reset=reset, choice=choice), record=record)
            greedy_tape = {
                'target_choice_u': bc(np.nan_to_num(ep['step/agent_tgt_choice_u'][s], nan=0.0)),
                'target_resample_u': bc(np.nan_to_num(ep['step/agent_tgt_binom_u'][s], nan=0.0)),
                'target_sample_u': bc(np.nan_to_num(ep['step/agent_tgt_sample_u'][s], nan=0.0)),
                'target_reset_sample_u': bc(np.nan_to_num(ep['agent/tgt_reset_sample_u'], nan=0.0)),
            }
            eng.step_versus_greedy('camera', bc(ep['step/cam_act'][s]), policy_tape=greedy_tape, tape_ct=bc(np.nan_to_num(ep['step/tape_ct'][s], nan=0.0)),
                                   tape_goal=bc(np.nan_to_num(ep['step/goal_u'][s], nan=0.0)), auto_reset=False)
            assert eng.last_flow not in ONE_LAUNCH_FLOWS
            assert record['choice'][1].tolist() == [kind] * N, (k, s)
            tgt_act = eng.policy_actions()[1].cpu().numpy()
            sd = eng.state_dict()
            for e in range(N):
                worst['target'] = max(worst['target'], np.abs(tgt_act[e] - ep['step/tgt_act'][s]).max())
                worst['xy'] = max(worst['xy'], np.abs(sd['tgt_x'][e] - ep['step/tgt_xy'][s][:, 0]).max(), np.abs(sd['tgt_y'][e] - ep['step/tgt_xy'][s][:, 1]).max())
            assert worst['target'] < 1e-8 and worst['xy'] < 1e-8, (k, s, names[int(ep['choice'][0])], worst)
            masks = eng.unpack_masks()
            assert np.array_equal(masks['camera_target_view_mask'][0], ep['step/camera_target_view_mask'][s]), (k, s)
            assert np.array_equal(sd['tgt_goals'][0], ep['step/tgt_goals'][s].astype(np.float64)), (k, s)
            assert np.array_equal(sd['bounties'][1], ep['step/bounties'][s].astype(np.float64)), (k, s)
            assert sd['episode_reward'][0] == ep['step/episode_reward'][s], (k, s)
    print('mixture_4v8-9:', [R.SCRIPTED_AGENTS[kind] for kind in played], 'worst differences', worst)
    assert len(played) == 8 and set(played) == {R.GREEDY, R.NAIVE, R.RANDOM}
