"""GPU tests of the communication trace (mate_engine_enable_comm_trace, csrc/trace_rows.hpp: comm_trace_kernel): the engine's
remaining[N, n, n] matrices against tests/render_comm_ref.py's rule driven by the engine's own delivered edges (Engine.channel_edges, Engine.message_edges) at
every step, bit for bit -- the 16-byte and the byte path, a tail tile, dropout, learner messages, restarts, seed() and import_state, graph replay, inertness,
the refusals, EngineGroups."""
import numpy as np
import pytest
import torch

import render_comm_ref as RC

pytestmark = pytest.mark.gpu

ESTATE, EINVAL = -4, -1
N = 33                 # two tiles of sixteen environments and a tail of one


def _config(config, **kw):
    import shape_edges
    from mate_amd.config import read_config
    if isinstance(config, tuple):
        return dict(shape_edges.scenario(config), **kw)
    return read_config(config, **kw)


def _engine(config, n=N, seed=23, policies=True, cut=25, **more):
    from mate_amd.engine import Engine
    eng = Engine(_config(config, max_episode_steps=cut), n, seed=seed, **more)
    if policies:
        eng.enable_policies()
    eng.reset()
    return eng


def _plant(eng):
    from test_gpu_scripted import _plant_emptied_warehouses
    return _plant_emptied_warehouses(eng)


class Wrapper:
    """RenderCommunication for a batch, on the host: one matrix and one episode tag per team and environment (the device's rule)."""

    def __init__(self, eng, teams, duration):
        self.duration, self.teams = duration, teams
        sizes = (eng.num_cameras, eng.num_targets)
        self.remaining = {t: np.zeros((eng.num_envs, sizes[t], sizes[t]), dtype=np.uint8) for t in teams}
        self.tags = {t: np.full(eng.num_envs, -1, dtype=np.int64) for t in teams}

    def before(self, eng, auto_reset, one_launch=False):
        """What the launch reads ahead of the step: which environments take a live step, and their episode numbers.  `one_launch`: the call is the one-launch
        step, which idles every finished environment whatever auto_reset is (its scalar record says done = 2)."""
        sd = eng.state_dict()
        self.live = ~((sd['done'] != 0) & (auto_reset > 1 or one_launch))
        self.episode = sd['episode'].astype(np.int64)

    def step(self, edges):
        """`edges`: {team: [N, n, n] of what was delivered since the previous step}."""
        for t in self.teams:
            for e in np.flatnonzero(self.live):
                if self.tags[t][e] != self.episode[e]:
                    self.remaining[t][e], self.tags[t][e] = 0, self.episode[e]
                self.remaining[t][e] = RC.trace_step(self.remaining[t][e], edges[t][e], self.duration)

    def check(self, eng, where):
        for t in self.teams:
            got = eng.communication_trace(t).cpu().numpy()
            assert got.dtype == np.uint8 and np.array_equal(got, self.remaining[t]), (where, t, np.argwhere(got != self.remaining[t])[:4].tolist())
            assert np.array_equal(eng.communication_trace_tags(t).cpu().numpy(), self.tags[t]), (where, t, 'tags')


def _delivered(eng, teams):
    torch.cuda.synchronize()
    return {t: eng.channel_edges(t)[1].cpu().numpy() != 0 for t in teams}


# ------------------------------------------------------------------ 1. the scripted agents' edges
@pytest.mark.parametrize('config,teams', [('MATE-4v8-9.yaml', (0, 1)), ('MATE-8v8-9.yaml', (0, 1)), ((12, 4, 3), (0, 1)), ((3, 5, 7), (0, 1)), ((1, 3, 2), (0, 1)),
                                          ('MATE-Navigation.yaml', (1,))], ids=['4v8-9', '8v8-9', '12v4-3', '3v5-7', '1v3-2', 'navigation'])
def test_the_trace_follows_the_delivered_edges_of_the_agents(config, teams):
    """60 Greedy-against-Greedy steps under the immediate restart (25-step episodes: every environment restarts twice): 16, 64 and 144 pairs on the 16-byte
    path, 9 and 25 pairs (and the single camera's one byte) on the byte path, no camera at all."""
    eng = _engine(config)
    if config == 'MATE-4v8-9.yaml':
        _plant(eng)      # (emptied warehouses: the targets talk)
    eng.enable_communication_trace(teams=teams, duration=20)
    assert all(eng.channels[t] is not None for t in teams)      # the transparent channels
    ref = Wrapper(eng, teams, 20)
    marks = 0
    for s in range(60):
        ref.before(eng, 1)
        eng.step_greedy(auto_reset=1)
        edges = _delivered(eng, teams)
        ref.step(edges)
        ref.check(eng, s)
        marks += sum(int(edges[t].sum()) for t in teams)
    assert marks > 0 or eng.num_cameras <= 1
    assert (ref.episode > 1).all()      # restarts happened, and the restarted environments started from zeros (check() at every step)


def test_under_dropout_the_trace_follows_delivered_not_sent():
    eng = _engine('MATE-4v8-9.yaml')
    _plant(eng)
    for t in (0, 1):
        eng.set_channel(t, dropout_rate=0.3)
    eng.enable_communication_trace(duration=7)
    assert eng.channels[0]['dropout_rate'] == 0.3      # the caller's channel stays
    ref, sent_only = Wrapper(eng, (0, 1), 7), 0
    for s in range(40):
        ref.before(eng, 1)
        eng.step_greedy(auto_reset=1)
        edges = _delivered(eng, (0, 1))
        sent_only += sum(int(((eng.channel_edges(t)[0].cpu().numpy() != 0) & ~edges[t]).sum()) for t in (0, 1))
        ref.step(edges)
        ref.check(eng, s)
    assert sent_only > 0


# ------------------------------------------------------------------ 2. the learner's messages
def _route(eng, team, address, gen, send):
    """A random address matrix, routed (or not: then the step_edges of the previous step are stale and must mark nothing)."""
    n = address.shape[1]
    address.copy_((torch.rand((eng.num_envs, n, n), generator=gen) < 0.2).to(torch.uint8).to(eng.device))
    if not send:
        return np.zeros((eng.num_envs, n, n), dtype=bool)
    eng.route_messages(team)
    torch.cuda.synchronize()
    return eng.message_edges(team)['step_edges'].cpu().numpy() > 0


@pytest.mark.parametrize('config', ['MATE-4v8-9.yaml', (3, 5, 7)], ids=['4v8-9', '3v5-7'])
def test_learner_messages_with_an_address_matrix(config):
    eng = _engine(config, policies=False)
    address = {t: eng.enable_messages(t, 2, addressed=True)[1] for t in (0, 1)}
    eng.enable_communication_trace(duration=5)
    assert eng.channels == [None, None]      # no on-device agents: no channel is installed
    ref = Wrapper(eng, (0, 1), 5)
    gen = torch.Generator(device='cpu').manual_seed(3)
    for s in range(40):
        ref.before(eng, 1)
        edges = {t: _route(eng, t, address[t], gen, send=(s + t) % 3 != 0) for t in (0, 1)}
        if s % 5 == 0:      # a second routing round between two steps: the deliveries of both count
            for t in (0, 1):
                if (s + t) % 3 != 0:
                    eng.route_messages(t, round=1)
                    torch.cuda.synchronize()
                    edges[t] = eng.message_edges(t)['step_edges'].cpu().numpy() > 0
        eng.step_random(auto_reset=1)
        ref.step(edges)
        ref.check(eng, s)
    assert all(ref.remaining[t].any() for t in (0, 1))


def test_learner_messages_together_with_a_scripted_teams_trace():
    """The learner plays the cameras and talks; the engine plays the Greedy targets under their transparent channel."""
    eng = _engine('MATE-4v8-9.yaml')
    _plant(eng)
    address = eng.enable_messages('camera', 3, addressed=True)[1]
    eng.enable_communication_trace(duration=20)
    ref = Wrapper(eng, (0, 1), 20)
    gen = torch.Generator(device='cpu').manual_seed(4)
    marks = 0
    for s in range(40):
        ref.before(eng, 1)
        mine = _route(eng, 0, address, gen, send=s % 2 == 0)
        action = ((torch.rand((N, eng.num_cameras, 2), generator=gen) * 2.0 - 1.0) * 3.0).to(eng.device)
        eng.step_versus_greedy('camera', action, auto_reset=1)
        theirs = _delivered(eng, (1,))[1]
        marks += int(theirs.sum())
        ref.step({0: mine, 1: theirs})
        ref.check(eng, s)
    assert marks > 0 and ref.remaining[0].any()


def test_the_one_launch_step_without_restarts_leaves_finished_environments_alone():
    """A trace on the caller's own team only: no live channel, so step_versus_greedy stays one launch, and with auto_reset = 0 every finished environment idles
    (done = 2): its matrix keeps its bytes, as the scalar record says."""
    eng = _engine('MATE-4v8-9.yaml', cut=5)
    address = eng.enable_messages('camera', 2, addressed=True)[1]
    eng.enable_communication_trace(teams=('camera',), duration=9)
    assert eng.channels[0] is not None and eng.channels[1] is None
    ref = Wrapper(eng, (0,), 9)
    gen = torch.Generator(device='cpu').manual_seed(6)
    idle_steps = 0
    for s in range(10):
        ref.before(eng, 0, one_launch=True)
        mine = _route(eng, 0, address, gen, send=True)
        action = ((torch.rand((N, eng.num_cameras, 2), generator=gen) * 2.0 - 1.0) * 3.0).to(eng.device)
        eng.step_versus_greedy('camera', action, auto_reset=0)
        torch.cuda.synchronize()
        assert eng.last_flow in (3, 4)      # FLOW_GREEDY / FLOW_STEP_GREEDY: the agents and the step in one kernel
        assert np.array_equal(eng.scalars[:, 2].cpu().numpy() == 2, ~ref.live), s
        idle_steps += int((~ref.live).sum())
        ref.step({0: mine})
        ref.check(eng, s)
    assert idle_steps > 0 and ref.remaining[0].any()


# ------------------------------------------------------------------ 3. restarts, seed(), import_state
def test_a_batched_restart_of_eight_leaves_idle_environments_alone():
    eng = _engine('MATE-4v8-9.yaml', cut=6)
    _plant(eng)
    eng.enable_communication_trace(duration=4)
    ref, idle_steps = Wrapper(eng, (0, 1), 4), 0
    for s in range(40):
        ref.before(eng, 8)
        idle_steps += int((~ref.live).sum())
        eng.step_greedy(auto_reset=8)
        ref.step(_delivered(eng, (0, 1)))
        ref.check(eng, s)
    assert idle_steps > 0 and (ref.episode > 1).all()


def test_seed_and_import_state_clear_the_trace():
    eng = _engine('MATE-4v8-9.yaml')
    eng.enable_communication_trace(duration=20)
    for _ in range(3):
        eng.step_greedy(auto_reset=1)
    torch.cuda.synchronize()
    assert eng.communication_trace('camera').any() and (eng.communication_trace_tags('camera') >= 0).all()
    exported = eng.export_state().clone()
    eng.seed(5)
    assert (eng.communication_trace_tags('camera') == -1).all() and (eng.communication_trace_tags('target') == -1).all()
    eng.reset()
    ref = Wrapper(eng, (0, 1), 20)
    for s in range(2):
        ref.before(eng, 1)
        eng.step_greedy(auto_reset=1)
        ref.step(_delivered(eng, (0, 1)))
        ref.check(eng, ('seed', s))
    eng.import_state(exported)
    torch.cuda.synchronize()
    assert (eng.communication_trace_tags('camera') == -1).all() and (eng.communication_trace_tags('target') == -1).all()
    ref = Wrapper(eng, (0, 1), 20)      # the same episode numbers as before the seed(): the cleared tags, not the numbers, start the matrices from zeros
    eng.observe()
    for s in range(2):
        ref.before(eng, 1)
        eng.step_greedy(auto_reset=1)
        ref.step(_delivered(eng, (0, 1)))
        ref.check(eng, ('import', s))


# ------------------------------------------------------------------ 4. graph replay, inertness
@pytest.mark.parametrize('versus', ['camera', 'target'])
def test_graph_replay_against_direct_calls(versus):
    K, team = 4, 0 if versus == 'camera' else 1
    # the engine's cameras talk all the time: ten-step episodes, batched restarts inside the graph; its targets only beside the planted emptied warehouses of
    # the first episode: one long episode and a duration that keeps their marks to the end
    cut, duration = (10, 6) if versus == 'target' else (60, 100)
    direct, graphed = (_engine('MATE-4v8-9.yaml', n=64, seed=9, cut=cut) for _ in range(2))
    action = ((torch.rand((64, (direct.num_cameras, direct.num_targets)[team], 2), generator=torch.Generator(device='cpu').manual_seed(2)) * 2.0 - 1.0) * 3.0).to(direct.device)
    for eng in (direct, graphed):
        _plant(eng)
        eng.enable_communication_trace(duration=duration)
    mine = action.clone()
    stepper = graphed.make_stepper(mine if team == 0 else None, mine if team == 1 else None, auto_reset=K, graph_steps=K, versus=versus)
    stepper.run(6 * K)
    torch.cuda.synchronize()
    for s in range(stepper.warmup_steps + 6 * K):
        direct.step_versus_greedy(versus, action, auto_reset=K)
    torch.cuda.synchronize()
    assert torch.equal(direct.scalars, graphed.scalars)
    for t in (0, 1):
        assert torch.equal(direct.communication_trace(t), graphed.communication_trace(t)) and torch.equal(direct.communication_trace_tags(t), graphed.communication_trace_tags(t))
    assert direct.communication_trace(1 - team).any()
    stepper.close()


def test_the_trace_changes_no_output_of_the_stepping_flows():
    """A twin with the same (transparent) channels and no trace: every output tensor of step_greedy, step_versus_greedy and step_selected, the records and
    the agents' joint actions are byte-equal."""
    def run(trace):
        eng = _engine('MATE-4v8-9.yaml', seed=11, cut=12)
        _plant(eng)
        for t in (0, 1):
            eng.set_channel(t)
        if trace:
            eng.enable_communication_trace(duration=20)
        selection = eng.enable_selection(True)
        gen = torch.Generator(device='cpu').manual_seed(5)
        seen = []
        for s in range(8):
            eng.step_greedy(auto_reset=1)
            seen.append([t.clone() for t in (eng.camera_obs, eng.target_obs, eng.scalars, eng.masks, eng.export_state(), *eng.policy_actions())])
            act = ((torch.rand((N, eng.num_targets, 2), generator=gen) * 2.0 - 1.0) * 20.0).to(eng.device)
            eng.step_versus_greedy('target', act, auto_reset=1)
            seen.append([t.clone() for t in (eng.camera_obs, eng.target_obs, eng.scalars, eng.export_state(), *eng.policy_actions())])
            selection.copy_(torch.randint(0, 256, (N, eng.num_cameras), generator=gen, dtype=torch.int32).to(eng.device))
            eng.step_selected(auto_reset=1)
            seen.append([t.clone() for t in (eng.camera_obs, eng.target_obs, eng.scalars, eng.export_state(), eng.selection_metrics)])
        return seen
    for s, (a, b) in enumerate(zip(run(False), run(True))):
        for x, y in zip(a, b):
            assert torch.equal(x, y), s


# ------------------------------------------------------------------ 5. the refusals, the groups
def test_every_refusal_changes_nothing():
    from mate_amd._native import EngineError
    eng = _engine('MATE-4v8-9.yaml', n=8)
    call = eng.lib.mate_engine_enable_comm_trace
    for mask, duration in ((3, 0), (3, 256), (1, -1), (4, 20), (-1, 20)):
        assert call(eng._h, mask, duration) == EINVAL, (mask, duration)
    with pytest.raises(EngineError) as err:
        eng.communication_trace('camera')
    assert err.value.code == ESTATE
    with pytest.raises(ValueError):
        eng.enable_communication_trace(duration=0)
    with pytest.raises(ValueError):
        eng.enable_communication_trace(duration=256)
    assert eng.channels == [None, None] and eng.trace_duration == 0      # a refused call installs no channel either
    nav = _engine('MATE-Navigation.yaml', n=4)
    assert nav.lib.mate_engine_enable_comm_trace(nav._h, 1, 20) == EINVAL and 'no cameras' in nav.lib.mate_engine_last_error().decode()
    with pytest.raises(ValueError):
        nav.enable_communication_trace()
    # the fused K-frame flows, and pipelined restarts, while a trace is enabled
    eng.enable_communication_trace(teams=('target',), duration=20)
    before = eng.export_state().clone()
    trace = eng.communication_trace('target').clone()
    for fused in (lambda: eng.rollout_random(2), lambda: eng.rollout_greedy(2), lambda: eng.rollout_greedy(2, auto_reset=-1),
                  lambda: eng.rollout_versus_greedy('camera', torch.zeros((8, eng.num_cameras, 2), device=eng.device), 2)):
        with pytest.raises(EngineError) as err:
            fused()
        assert err.value.code == ESTATE and 'step per frame' in str(err.value)
    torch.cuda.synchronize()
    assert torch.equal(before, eng.export_state()) and torch.equal(trace, eng.communication_trace('target'))
    with pytest.raises(EngineError):
        eng.communication_trace('camera')      # not in the mask
    wrong = torch.zeros((8, 3, 3), dtype=torch.uint8, device=eng.device)
    with pytest.raises(ValueError):
        eng.set_communication_trace('target', wrong)
    eng.disable_communication_trace()
    eng.clear_channel('target')
    eng.rollout_greedy(2)      # detached: the fused flows are back
    eng.rollout_greedy(2, auto_reset='pipelined')
    eng.enable_communication_trace(teams=('camera',), duration=3)      # enabling leaves the pipelined-restart mode, as every attachment does; the next pipelined call is refused
    with pytest.raises(EngineError) as err:
        eng.rollout_greedy(2, auto_reset='pipelined')
    assert err.value.code == ESTATE
    eng.disable_communication_trace()
    eng.clear_channel('camera')
    with pytest.raises(EngineError):
        eng.set_communication_trace('target', torch.zeros((8, 8, 8), dtype=torch.uint8, device=eng.device))


def test_two_engine_groups_against_one_engine():
    from mate_amd.engine import EngineGroups
    cfg = _config('MATE-4v8-9.yaml', max_episode_steps=10)
    groups = EngineGroups(cfg, 32, groups=2, seed=41, policies=True)
    groups.reset()
    single = _engine('MATE-4v8-9.yaml', n=32, seed=41, cut=10)
    groups.enable_communication_trace(duration=9)
    single.enable_communication_trace(duration=9)
    for s in range(25):
        groups.each(lambda g, eng: eng.step_greedy(auto_reset=1))
        single.step_greedy(auto_reset=1)
    groups.synchronize()
    torch.cuda.synchronize()
    for team in ('camera', 'target'):
        assert torch.equal(torch.cat(groups.communication_trace(team)), single.communication_trace(team)), team
    assert single.communication_trace('camera').any()
    groups.close()
