"""The attached launches all at once: the cases, the builder of FULL / ONE / BARE engines and the comparison helpers shared by
tests/test_gpu_stack.py (the HIP engine) and tests/test_stack_cases_cpu.py (is the plan real: do the names exist, do the seeds draw every
candidate, do the straddling rows fill?).  Both take their cases from CASES, so what was counted is what is compared.

Actors change the trajectory: the flow itself (step_selected's executor among them), set_camera_opponent, set_opponent_mixture,
set_channel, the sub-wave switch.  Observers only read: reward rows (with terms), info rows, selection metrics and action mask, fragment
rows with first rows and final_obs, episode records, state rows.  Everything the engine draws is Philox-keyed by (seed, global
environment, episode, tick), so engines built alike walk the same trajectory whatever observes them:

  FULL     every observer of the case attached;
  ONE[o]   observer o alone -- with the observer it reads by design: episode records come with the reward rows (per-step flows) or the
           fragment rows (FrameSkip) whose shaped row they sum;
  BARE     nothing attached.

A session that calls step_selected needs enable_selection on every engine (the call is refused without it): there the executor is part
of the actor configuration, BARE carries it, and BARE is ONE['selection'].

Equality is by bits (launch_forms.same).  The restatement checks on FULL import their references and bars from the features' own files."""
import collections

import numpy as np

import shape_edges as S

MATE_EINVAL, MATE_ESTATE = -1, -4
K = 3                                      # frames of the fused flows
OBSERVERS = ('reward', 'info', 'selection', 'episodes', 'state', 'fragment')
ENABLE = {'reward': 'enable_reward_rows', 'info': 'enable_info_rows', 'selection': 'enable_selection', 'episodes': 'enable_episode_records',
          'state': 'enable_state_rows', 'fragment': 'enable_fragment_rows'}
DISABLE = {'reward': 'disable_reward_rows', 'info': 'disable_info_rows', 'selection': 'disable_selection', 'episodes': 'disable_episode_records',
           'state': 'disable_state_rows', 'fragment': 'disable_fragment_rows'}
ACTORS = {'target_mixture': 'set_opponent_mixture', 'camera_mixture': 'set_opponent_mixture', 'target_channel': 'set_channel',
          'camera_channel': 'set_channel', 'sub_wave': 'set_sub_wave'}
# the second phase of the target learner's case (tests/test_gpu_stack.py _switch_to_heuristic_cameras)
SWITCHES = ('clear_opponent_mixture', 'clear_channel', 'set_camera_opponent', 'set_channel')
Flow = collections.namedtuple('Flow', 'method frames agents team')
FLOWS = {
    'step': Flow('step', 1, False, None), 'step_random': Flow('step_random', 1, False, None), 'step_greedy': Flow('step_greedy', 1, True, None),
    'versus_camera': Flow('step_versus_greedy', 1, True, 'camera'), 'versus_target': Flow('step_versus_greedy', 1, True, 'target'),
    'step_selected': Flow('step_selected', 1, True, None), 'rollout_random': Flow('rollout_random', K, False, None),
    'skip_camera': Flow('rollout_versus_greedy', K, True, 'camera'), 'skip_target': Flow('rollout_versus_greedy', K, True, 'target'),
}
PER_STEP = ('step', 'step_random', 'step_greedy', 'versus_camera', 'versus_target', 'step_selected', 'rollout_random')
RESTATEMENTS = ('info', 'episodes', 'state', 'channel', 'mixture', 'reward')

TARGET_MIXTURE = {'greedy': 1.0, 'heuristic': 1.0, 'naive': 1.0, 'random': 1.0}
CAMERA_MIXTURE = {'greedy': 1.0, 'naive': 1.0, 'random': 1.0}
CHANNEL = {'dropout_rate': 0.3, 'range_limit': 1400.0}
S_SCR_CHOICE = 22                          # csrc/scripted_rows.hpp: the mixture draw's stream, counter (environment, episode, stream, team)
FRAGMENT_SHAPING = {'camera': ({'coverage_rate': 1.0, 'num_tracked': 0.25}, 'mean'), 'target': ({'raw_reward': 1.0, 'is_tracked': -0.5}, 'none')}

Case = collections.namedtuple('Case', 'name section scenario n cut seed first dtype flows observers episodes_team actors regime skips why')


def _case(name, section, scenario, n, cut, dtype, flows, observers, why, episodes_team='camera', actors=None, regime=1, skips=(), seed=4401, first=7):
    return Case(name, section, scenario, n, cut, seed, first, dtype, tuple(flows), tuple(observers), episodes_team, dict(actors or {}), regime, tuple(skips), why)


STEP_OBSERVERS = ('reward', 'info', 'selection', 'episodes', 'state')
SKIP_OBSERVERS = ('fragment', 'episodes', 'info', 'state')
SHAPES = (('MATE-4v8-9', 40), ('7v5-3', 41))      # two full attached tiles and a half one, specialised; view rows that straddle a word, generic
CASES = []
# 1: the observers behind every per-step flow, three restart regimes (0: the caller's masked reset, 1: immediate, 3: batched with
#    auto_reset = 1 calls inside open intervals).  No channel and no mixture here: those two restatements belong to section 2.
for _scenario, _n in SHAPES:
    for _dtype in ('f32', 'f64'):
        for _regime in (0, 1, 3):
            CASES.append(_case('flows_%s_%s_reset%d' % (_scenario, _dtype, _regime), 1, _scenario, _n, 7, _dtype, PER_STEP, STEP_OBSERVERS,
                               'every flow behind every other with all observers; rows that read rows (5c reads 3), two snapshots behind one restart (6c)',
                               regime=_regime, skips=('channel', 'mixture')))
# 2: the actor stacks
for _scenario, _n in SHAPES:
    CASES.append(_case('camera_learner_' + _scenario, 2, _scenario, _n, 6, 'f32', ('versus_camera', 'step_selected'), STEP_OBSERVERS,
                       'the agents\' launch of the two-launch form under a mixture and a lossy channel, q.caller_team, with the four observers behind it',
                       actors={'target_mixture': TARGET_MIXTURE, 'target_channel': CHANNEL}))
    CASES.append(_case('target_learner_' + _scenario, 2, _scenario, _n, 6, 'f32', ('versus_target',), STEP_OBSERVERS,
                       'a camera mixture under a camera channel, then the Heuristic cameras with the (inert) channel of the caller\'s own team',
                       episodes_team='target', actors={'camera_mixture': CAMERA_MIXTURE, 'camera_channel': CHANNEL}))
# 3: FrameSkip -- no reward rows (the fragment's shaped row is the learner's), no channel, no mixture (the fused launch holds the Greedy agents)
for _scenario, _n in SHAPES:
    for _team in ('camera', 'target'):
        for _regime in (1, 2):
            CASES.append(_case('frameskip_%s_%s_reset%d' % (_team, _scenario, _regime), 3, _scenario, _n, 7, 'f32', ('skip_' + _team,), SKIP_OBSERVERS,
                               'fragment (5), first rows (5b, 6b), records (5c) and info rows (3b, 6c) behind one K-frame launch', episodes_team=_team,
                               regime=_regime, skips=('channel', 'mixture', 'reward')))
# 4: the one-step form of the sub-wave rollout kernel
CASES.append(_case('sub_wave_MATE-2v4-0', 4, 'MATE-2v4-0', 24, 7, 'f32', ('step_random', 'step_greedy', 'versus_target'), STEP_OBSERVERS,
                   'E = 4 environments per wave under the attached launches', actors={'sub_wave': True}, skips=('channel', 'mixture')))
# 5: all maxima, observers only (no on-device agents among 64 obstacles: no selection, and no soft coverage score -- no test holds the
#    outer occlusion boundary among 64 obstacles to a reference)
CASES.append(_case('all_maxima_16v16-64', 5, '16v16-64', 8, 5, 'f32', ('step_random',), ('reward', 'info', 'episodes', 'state'),
                   'state-rows tile of E = 4 beside info and reward tiles of 16', skips=('channel', 'mixture'), seed=4301))


def case(name):
    return {c.name: c for c in CASES}[name]


def cases_of(section):
    return [c for c in CASES if c.section == section]


def has_policies(c):
    return c.scenario != '16v16-64'


def edge_case(c):
    """The case of shape_edges.ATTACHED_CASES a generic scenario names (None for a shipped one)."""
    return None if c.scenario.startswith('MATE-') else S.attached_case(c.scenario)


def config_of(c):
    from mate_amd.config import read_config
    if c.scenario.startswith('MATE-'):
        return read_config(c.scenario + '.yaml', max_episode_steps=c.cut)
    return read_config(S.case_scenario(edge_case(c)), max_episode_steps=c.cut)


def pairs(c, observer):
    """What ONE[observer] attaches."""
    if observer == 'episodes':
        return ('fragment', 'episodes') if 'fragment' in c.observers else ('reward', 'episodes')
    return (observer,)


def euler_order(flows):
    """A closed walk over the flows in which every flow follows every other exactly once: for a prime count n the n - 1 cycles
    0, d, 2d, ... (mod n), each back at 0."""
    n = len(flows)
    assert n in (2, 3, 5, 7)
    order = [0]
    for d in range(1, n):
        order += [(d * k) % n for k in range(1, n + 1)]
    return [flows[i] for i in order]


def mixture_uniform(O, seed, env_global, episode, team):
    """The uniform of the mixture draw of (environment, episode, team) as csrc/scripted_kernels.hip takes it: u53 of the first two words of
    philox(seed, (environment, episode, S_SCR_CHOICE, team))."""
    x, y = O.philox(seed & 0xffffffff, seed >> 32, int(env_global), int(episode), S_SCR_CHOICE, int(team))[:2]
    return (float(x >> 5) * 67108864.0 + float(y >> 6)) * (1.0 / 9007199254740992.0)


def mixture_choices(O, c, mixture, team, episodes):
    """[len(episodes), n] names' indices (SCRIPTED_AGENTS) the case's seed draws for the team: scripted_ref.mixture_choice on the oracle's Philox."""
    import scripted_ref
    names = [name for name, w in mixture.items() if w > 0.0]
    kinds = np.array([scripted_ref.SCRIPTED_AGENTS.index(name) for name in names])
    u = np.array([[mixture_uniform(O, c.seed, c.first + e, episode, team) for e in range(c.n)] for episode in episodes])
    return kinds[scripted_ref.mixture_choice([mixture[name] for name in names], u)]


# ---------------------------------------------------------------------------------------------- engines (GPU)
def row_dtype(c):
    import torch
    return torch.float64 if c.dtype == 'f64' else torch.float32


def reward_specs(c, eng):
    from test_gpu_reward_rows import CAMERA_COEFFICIENTS, TARGET_COEFFICIENTS
    cam, tgt = dict(CAMERA_COEFFICIENTS), dict(TARGET_COEFFICIENTS)
    if c.scenario == '16v16-64':
        cam.pop('soft_coverage_score'), tgt.pop('soft_coverage_score')
    return ((cam, 'mean') if eng.num_cameras else None), (tgt, 'none')


def attach(eng, c, which):
    """The observers `which`, in the order BatchedMultiAgentTracking.reset attaches them."""
    if 'state' in which:
        eng.enable_state_rows()
    if 'reward' in which:
        cam, tgt = reward_specs(c, eng)
        eng.enable_reward_rows(camera=cam, target=tgt, dtype=row_dtype(c), terms=True)
    if 'selection' in which:
        eng.enable_selection(True, accumulate=True)
    if 'info' in which:
        eng.enable_info_rows()
    if 'fragment' in which:
        eng.enable_fragment_rows(c.episodes_team, K, shaping=FRAGMENT_SHAPING[c.episodes_team], dtype=row_dtype(c), first_rows=True, final_obs=True)
    if 'episodes' in which:
        eng.enable_episode_records(c.episodes_team)


def detach(eng, observer):
    getattr(eng, DISABLE[observer])()


def apply_actors(eng, actors):
    for team in ('camera', 'target'):
        if team + '_mixture' in actors:
            eng.set_opponent_mixture(team, actors[team + '_mixture'])
        if team + '_channel' in actors:
            eng.set_channel(team, **actors[team + '_channel'])


LIVE = []                                   # the engines build() made and close_all() has not destroyed yet


def close_all():
    """Destroy every engine build() made, now: mate_engine_destroy waits for the device and frees, which must not be left to whenever the
    collector finds an engine -- possibly inside a later test's stream capture.  tests/test_gpu_stack.py calls this behind every test."""
    while LIVE:
        LIVE.pop().close()


def build(c, which, stagger=True):
    """An engine of the case with its actors, reset, its environments' episodes staggered over four phases (a time limit would end them
    all in one call), then the observers `which`."""
    import torch
    from mate_amd.engine import Engine
    eng = Engine(config_of(c), c.n, seed=c.seed, first_env_index=c.first, obs_dtype=row_dtype(c))
    assert eng.specialised == c.scenario.startswith('MATE-'), c.name
    if has_policies(c):
        eng.enable_policies()
    if c.actors.get('sub_wave'):
        assert eng.set_sub_wave(True) == 4
    apply_actors(eng, c.actors)
    eng.reset()
    if stagger:
        phase = torch.arange(c.n, device=eng.device) % 4
        for k in (1, 2, 3):
            eng.step_random(auto_reset=0, want_masks=True)
            eng.reset(env_mask=phase == k)
    LIVE.append(eng)
    attach(eng, c, which)
    return eng


def same(a, b):
    from launch_forms import same as same_bits
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and same_bits(a, b)


def first_difference(a, b):
    """Where two tensors of one shape first differ by bits, and the two values there (for an assertion's message)."""
    if a is None or b is None or a.shape != b.shape or a.dtype != b.dtype:
        return 'shapes or types differ'
    import torch
    x, y = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    size = x.element_size()
    differs = (x.view(torch.uint8).reshape(-1, size) != y.view(torch.uint8).reshape(-1, size)).any(dim=1).nonzero().reshape(-1)
    if len(differs) == 0:
        return 'equal'
    i = int(differs[0])
    index = [int(v) for v in np.unravel_index(i, tuple(a.shape))]
    return '%d elements differ, first at %s: %r (bytes %s) != %r (bytes %s)' % (len(differs), index, x[i].item(), bytes(x[i:i + 1].view(torch.uint8).tolist()).hex(),
                                                                          y[i].item(), bytes(y[i:i + 1].view(torch.uint8).tolist()).hex())


def outputs(eng, observer):
    """{name: tensor or None} of what the observer leaves (the episode records apart: Stack.records)."""
    names = {'reward': ('camera_reward_rows', 'target_reward_rows', 'camera_reward_terms', 'target_reward_terms'),
             'info': ('info_camera_rows', 'info_target_rows', 'info_cargo_rows'),
             'selection': ('selection_metrics', 'selection_frames', 'action_mask', 'selection_actions'), 'state': ('state',), 'episodes': ()}
    if observer == 'fragment':
        out = {k: v for k, v in eng.fragment.items()}
        out['restarted'] = eng.fragment_restarted
        return out
    return {name: getattr(eng, name) for name in names[observer]}


def trajectory(eng, c, flow, ret):
    """{name: tensor} of what a call of `flow` returned and left: rows, scalars, masks, the exported state, and where agents acted their
    actions, memory and edge matrices."""
    f = FLOWS[flow]
    if f.frames > 1:
        out = {'camera_obs': ret[0], 'target_obs': ret[1], 'scalars': ret[2], 'masks': eng._rollout['masks'][:f.frames]}
    else:
        out = {'camera_obs': eng.camera_obs, 'target_obs': eng.target_obs, 'scalars': eng.scalars, 'masks': eng.masks}
    out['state'] = eng.export_state()
    if f.agents:
        out['camera_actions'], out['target_actions'] = eng.policy_actions()
        for team in (0, 1):
            if eng.mixtures[team] is not None:
                out.update({'memory %d %s' % (team, k): v for k, v in eng.scripted_memory(team).items()})
                out['greedy rows %d' % team] = eng.scripted_rows(team, 'greedy')
            if eng.channels[team] is not None:
                out['sent %d' % team], out['delivered %d' % team] = eng.channel_edges(team)
    return out


class Stack:
    """FULL, BARE and the ONE engines of a case, called together and compared after every call."""

    def __init__(self, c, ones=True):
        import torch
        self.c = c
        self.base = ('selection',) if 'step_selected' in c.flows else ()
        assert set(c.observers) <= set(OBSERVERS) and set(self.base) <= set(c.observers)
        self.full, self.bare = build(c, c.observers), build(c, self.base)
        self.one = {o: build(c, self.base + tuple(x for x in pairs(c, o) if x not in self.base)) for o in c.observers if o not in self.base} if ones else {}
        for o in self.base:
            self.one[o] = self.bare
        self.attached = {o: True for o in c.observers}
        self.calls = 0
        self.gen = torch.Generator(device='cpu').manual_seed(c.seed)
        self.records = {'full': [], 'one': []}
        self.dropped = 0

    @property
    def engines(self):
        seen, out = set(), []
        for eng in [self.full, self.bare] + list(self.one.values()):
            if id(eng) not in seen:
                seen.add(id(eng))
                out.append(eng)
        return out

    def each(self, fn):
        return [fn(eng) for eng in self.engines]

    def actions(self):
        """This call's f32 joint actions and selection words, the same for every engine."""
        import torch
        eng = self.full
        n, nc, nt = eng.num_envs, eng.num_cameras, eng.num_targets
        cam = ((torch.rand((n, nc, 2), generator=self.gen) * 2 - 1) * 5.0).to(eng.device)
        tgt = ((torch.rand((n, nt, 2), generator=self.gen) * 2 - 1) * 20.0).to(eng.device)
        words = ((torch.arange(n * nc).view(n, nc) * 7 + self.calls * 13) % (1 << nt)).to(torch.int32).to(eng.device)
        return cam, tgt, words

    @staticmethod
    def invoke(eng, flow, auto_reset, cam, tgt, words):
        f = FLOWS[flow]
        if eng.selection is not None:
            eng.selection.copy_(words)
        if flow == 'step':
            return eng.step(cam, tgt, auto_reset=auto_reset)
        if flow == 'step_random':
            return eng.step_random(auto_reset=auto_reset, want_masks=True)
        if flow in ('step_greedy', 'step_selected'):
            return getattr(eng, f.method)(auto_reset=auto_reset)
        if flow == 'rollout_random':
            return eng.rollout_random(K, auto_reset=auto_reset, want_masks=True)
        action = cam if f.team == 'camera' else tgt
        if f.frames > 1:
            return eng.rollout_versus_greedy(f.team, action, K, auto_reset=auto_reset, want_masks=True)
        return eng.step_versus_greedy(f.team, action, auto_reset=auto_reset)

    def call(self, flow, auto_reset, compare=True):
        """One call of `flow` on every engine; returns FULL's return value."""
        cam, tgt, words = self.actions()
        rets = {id(eng): self.invoke(eng, flow, auto_reset, cam, tgt, words) for eng in self.engines}
        self.calls += 1
        if compare:
            self.compare(flow, rets, (self.c.name, self.calls, flow, auto_reset))
        return rets[id(self.full)]

    def compare_observers(self, where):
        for o, eng in self.one.items():
            if not self.attached[o]:
                continue
            for name, x in outputs(self.full, o).items():
                y = outputs(eng, o)[name]
                assert same(x, y), (where, 'FULL differs from ONE[%s]' % o, name, first_difference(x, y))
        if 'episodes' in self.one and self.attached['episodes']:
            import episode_ref
            (full, dropped_full), (one, dropped_one) = self.full.episode_records(), self.one['episodes'].episode_records()
            full, one = full.cpu().numpy(), one.cpu().numpy()
            assert dropped_full == dropped_one and full.shape == one.shape, (where, 'record counts')
            if len(full):
                assert episode_ref.same_bits(episode_ref.sort_records(full), episode_ref.sort_records(one)), (where, 'FULL differs from ONE[episodes]')
            self.records['full'].extend(full)
            self.dropped += dropped_full

    def compare_trajectory(self, flow, rets, where):
        ref = trajectory(self.bare, self.c, flow, rets[id(self.bare)])
        for eng in self.engines:
            if eng is self.bare:
                continue
            got = trajectory(eng, self.c, flow, rets[id(eng)])
            assert got.keys() == ref.keys()
            for name in ref:
                assert same(got[name], ref[name]), (where, 'FULL' if eng is self.full else 'a ONE engine', 'differs from BARE', name, first_difference(got[name], ref[name]))

    def compare(self, flow, rets, where):
        self.compare_trajectory(flow, rets, where)
        self.compare_observers(where)

    def reset_finished(self, done):
        self.each(lambda eng: eng.reset(env_mask=done))

