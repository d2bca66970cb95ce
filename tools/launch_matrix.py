#!/usr/bin/env python3
"""A profiling target: every stepping entry point in every launch form the host can plan (csrc/engine_host.h: plan_step,
plan_rollout_random, plan_with_policies), as one fixed list of calls.  One line per call: the flow the launch ran (Engine.last_flow) and
the environments per wave the Greedy rollouts run with (Engine.sub_wave), or the engine's error code where the call is rejected.
python tools/launch_matrix.py [<shape> [<batch>]]      (default: every shape at both batches)
Under `rocprofv3 --kernel-trace -- python tools/launch_matrix.py ...` the ordered (kernel, grid, workgroup, LDS) list of two builds of
the library (MATE_ENGINE_LIB) must be the same; tests/test_gpu_launch_matrix.py runs the 8-environment part against recorded values.
The environment switches are read when an engine is created: a column under one of SWITCH_COLUMNS is run with the variable set.
python tools/launch_matrix.py attached [<shape>]      the ATTACHED column set: every call that leaves new records under every combination of
attached launches (state rows, reward rows, target selection), and the calls the engine refuses, each on an engine of its own;
`attached --record PATH` writes the record (status, error text, SHA-256 of every attached output and of export_state() per call) as JSON:
the record of two builds of the library (MATE_ENGINE_LIB) must be the same bytes.
python tools/launch_matrix.py opponents               the OPPONENTS column set: every per-step and fused call with the on-device agents under the opponent
selections, mixtures and channels the setters can reach (one engine per shape, reconfigured between states), and the setters' refusals; per call the
status, the error text, the flow, which buffer policy_actions() equals and whether the channel edges changed (tests/golden/opponent_flows.json);
`opponents --golden PATH --commit ID` writes that file; `opponents --record PATH` adds the SHA-256 of every output, of policy_actions, scripted_memory, the channel edges and export_state(): the same bytes
from two builds of the library.
python tools/launch_matrix.py host-cost [<batch>]     microseconds of host time and per graph-replayed step of step_versus_greedy and
step_selected with all three attached (default: 4096 environments of MATE-4v8-9)."""
import hashlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, 'tests')):
    if path not in sys.path:
        sys.path.insert(0, path)
from mate_amd._native import EngineError  # noqa: E402
from mate_amd.config import read_config  # noqa: E402
from mate_amd.engine import Engine  # noqa: E402

# E = 4 everywhere | the random flow stays one per wave in auto mode | E = 2, Greedy flows only | row image, E = 1 | generic kernels (tests/shape_edges.py)
SHAPES = ('MATE-2v4-0', 'MATE-4v4-9', 'MATE-4v8-0', 'MATE-4v8-9', '3v5-7')
# every shape with sub-wave kernels (engine_kernels.hpp sub_wave_of: at most four cameras and four targets, and MATE-4v8-0) + the rest of SHAPES
IN_USE_SHAPES = tuple('MATE-%s-%d' % (s, o) for s in ('1v1', '1v2', '2v2', '2v4', '4v2', '4v4') for o in (0, 9)) + ('MATE-4v8-0', 'MATE-4v8-9', '3v5-7')
SMALL_BATCH = 8                      # split-kernel territory; the auto threshold: 32 environments per compute unit (threshold_batch)
DTYPES = ('f32', 'f64')
MODES = (False, True, 'auto')        # Engine.set_sub_wave
AUTO_RESETS = (0, 1, 3)
ROLLOUT_STEPS = 3
CALLS = ('step', 'step_random', 'rollout_random', 'step_greedy', 'step_greedy_tape', 'step_versus_greedy_camera', 'step_versus_greedy_target',
         'rollout_greedy', 'rollout_versus_greedy_camera', 'rollout_versus_greedy_target')
CALL_LIST = [('observe', 0)] + [(name, k) for name in CALLS for k in AUTO_RESETS]
# the small-batch MATE-2v4-0 column again under each of these (read at create)
SWITCH_COLUMNS = ('MATE_STEP_SUBWAVE=0', 'MATE_STEP_GREEDY_ROLLOUT=1', 'MATE_POLICY_SPLIT=1', 'MATE_STEP_SPLIT=0', 'MATE_STEP_SPLIT=1')


def threshold_batch():
    return 32 * torch.cuda.get_device_properties(0).multi_processor_count


def config_of(shape):
    if shape.startswith('MATE-'):
        return read_config(shape + '.yaml', max_episode_steps=7)
    import shape_edges
    nc, rest = shape.split('v')
    nt, no = rest.split('-')
    return read_config(dict(shape_edges.scenario((int(nc), int(nt), int(no))), max_episode_steps=7))


def make_engine(shape, batch, dtype, transform, mode):
    """(engine, in_use): policies on, reset, rollout buffers reserved; `in_use`: what set_sub_wave(mode) answered."""
    eng = Engine(config_of(shape), batch, seed=11, first_env_index=2, obs_dtype=torch.float64 if dtype == 'f64' else torch.float32)
    in_use = eng.set_sub_wave(mode)
    eng.enable_policies()
    if transform:
        eng.set_obs_transform(relative_coordinates=True)
    eng.reset()
    eng.reserve_rollout(ROLLOUT_STEPS, want_masks=True, search='none')
    return eng, in_use


def actions_of(eng):
    gen = torch.Generator().manual_seed(7)
    cam = ((torch.rand((eng.num_envs, eng.num_cameras, 2), generator=gen) * 2 - 1) * torch.tensor([5.0, 2.5])).to(eng.device)
    tgt = ((torch.rand((eng.num_envs, eng.num_targets, 2), generator=gen) * 2 - 1) * 20.0).to(eng.device)
    tape = {'target_choice_u': torch.full((eng.num_envs, eng.num_targets), 0.5, dtype=torch.float64, device=eng.device)}
    return cam, tgt, tape


def issue(eng, name, k, acts):
    """One call of CALL_LIST; returns the tensors it wrote."""
    cam, tgt, tape = acts
    if name == 'observe':
        return eng.observe()
    if name == 'step':
        return eng.step(cam, tgt, auto_reset=k)
    if name == 'step_random':
        return eng.step_random(auto_reset=k, want_masks=True)
    if name == 'rollout_random':
        return eng.rollout_random(ROLLOUT_STEPS, auto_reset=k, want_masks=True)
    if name == 'step_greedy':
        return eng.step_greedy(auto_reset=k)
    if name == 'step_greedy_tape':
        return eng.step_greedy(policy_tape=tape, auto_reset=k)
    if name == 'rollout_greedy':
        return eng.rollout_greedy(ROLLOUT_STEPS, auto_reset=k, want_masks=True)
    kind, team = name.rsplit('_', 1)
    mine = cam if team == 'camera' else tgt
    if kind == 'step_versus_greedy':
        return eng.step_versus_greedy(team, mine, auto_reset=k)
    assert kind == 'rollout_versus_greedy', name
    return eng.rollout_versus_greedy(team, mine, ROLLOUT_STEPS, auto_reset=k, want_masks=True)


def run_column(eng):
    """Issues CALL_LIST on `eng`; yields (call id, [last_flow, sub_wave, error code], outputs or None) behind each call."""
    acts = actions_of(eng)
    for name, k in CALL_LIST:
        code, out = 0, None
        try:
            out = issue(eng, name, k, acts)
        except EngineError as err:
            code = err.code
        yield '%s/%d' % (name, k), [eng.last_flow, eng.sub_wave, code], out


def column_id(shape, dtype, transform, mode):
    return '%s %s %s sub_wave=%s' % (shape, dtype, 'transform' if transform else 'plain', mode)


def small_batch_record(shape, compare=None):
    """{column id: [[last_flow, sub_wave, error code] of every call of CALL_LIST]}: the 8-environment columns of `shape`, the three modes of
    a column stepped side by side.  compare(what, engine of set_sub_wave(False), its outputs, engine of (True), its outputs) behind each call."""
    record = {}
    for dtype in DTYPES:
        for transform in (False, True):
            engines = [make_engine(shape, SMALL_BATCH, dtype, transform, mode)[0] for mode in MODES]
            rows = [[] for _ in MODES]
            for results in zip(*[run_column(eng) for eng in engines]):
                for row, (_, values, _) in zip(rows, results):
                    row.append(values)
                if compare:
                    compare('%s %s' % (column_id(shape, dtype, transform, 'False/True'), results[0][0]), engines[0], results[0][2], engines[1], results[1][2])
            torch.cuda.synchronize()
            for mode, row, eng in zip(MODES, rows, engines):
                record[column_id(shape, dtype, transform, mode)] = row
                eng.close()
    return record


def in_use_record(shape):
    """{'small' | 'threshold': [set_sub_wave(mode) for the three modes, ahead of enable_policies() | behind it]}"""
    record = {}
    for label, batch in (('small', SMALL_BATCH), ('threshold', threshold_batch())):
        eng = Engine(config_of(shape), batch, seed=11)
        before = [eng.set_sub_wave(mode) for mode in MODES]
        eng.enable_policies()
        record[label] = [before, [eng.set_sub_wave(mode) for mode in MODES]]
        eng.close()
    return record


# ---- the attached column set
ATTACHED_SHAPES = ('MATE-2v4-0', 'MATE-4v8-9')      # (the 32 camera->target bits of MATE-4v8-9 straddle mask words)
ATTACHED_BATCH = 17                                  # one full 16-environment tile and a second tile holding one environment
ATTACHED = ('state', 'reward', 'reward_soft', 'selection_multi', 'selection_single', 'all')
STEPPING = ('step', 'step_random', 'step_greedy', 'step_versus_greedy_camera', 'step_versus_greedy_target', 'step_selected',
            'rollout_random', 'rollout_greedy', 'rollout_versus_greedy_camera', 'rollout_versus_greedy_target')
# (auto_reset = 3 is issued four times: the third call ends the interval, the fourth opens one the next flow has to flush)
ATTACHED_CALLS = ([('reset', 0), ('reset_masked', 0), ('observe', 0)] +
                  [(name, k) for k in AUTO_RESETS for name in STEPPING for _ in range(4 if k == 3 else 1)] +
                  [('import_state', 0), ('step_selected', 1), ('observe', 0), ('device_tick_on', 3), ('step_random', 3), ('device_tick_off', 0)])
ATTACHED_OUTPUTS = ('camera_reward_rows', 'target_reward_rows', 'camera_reward_terms', 'target_reward_terms', 'selection_actions',
                    'selection_metrics', 'selection_frames', 'action_mask', 'state')
CAMERA_TERMS = {'coverage_rate': 1.0, 'num_tracked': 0.25, 'baseline': -0.5}
TARGET_TERMS = {'raw_reward': 1.0, 'normalized_goal_distance': -1.0, 'sparse_delivery': 10.0, 'is_tracked': -0.5, 'is_colliding': -1.0}
SOFT_TERM = {'soft_coverage_score': 0.125}
# the calls the engine refuses: (id, what is attached, the calls in front, the refused call)
REFUSED = ([('pipelined under ' + combo, combo, (), 'rollout_greedy_pipelined') for combo in ('state', 'reward', 'selection_multi', 'all')] +
           [('%s under reward' % call, 'reward', (), call) for call in ('step_random_no_masks', 'step_random_no_scalars', 'rollout_random_no_masks',
                                                                         'rollout_greedy_no_masks', 'step_greedy_no_masks')] +
           [('step_selected behind rollout_random', 'selection_multi', (('rollout_random', 1),), 'step_selected'),
            ('step_selected behind import_state', 'selection_multi', (('import_state', 0),), 'step_selected'),
            ('step_selected without policies', 'none', (), 'step_selected_no_policies'),
            ('step_selected without masks under reward', 'all', (), 'step_selected_no_masks')])


def attach(eng, combo):
    """Attaches `combo` to a reset engine with policies on; 'all' turns every option the other columns leave off."""
    everything = combo == 'all'
    gen = torch.Generator().manual_seed(5)
    if combo.startswith('reward') or everything:
        soft = SOFT_TERM if combo == 'reward_soft' or everything else {}
        eng.enable_reward_rows(camera=(dict(CAMERA_TERMS, **soft), 'mean'), target=(dict(TARGET_TERMS, **soft), 'none'), terms=True,
                               dtype=torch.float32 if everything else torch.float64, accumulate=everything)
    if combo.startswith('selection') or everything:
        multi = combo != 'selection_single'
        high = (1 << eng.num_targets) if multi else eng.num_targets + 1
        selection = torch.randint(0, high, (eng.num_envs, eng.num_cameras), generator=gen).to(dtype=torch.int32, device=eng.device)
        eng.enable_selection(multi_selection=multi, selection=selection, accumulate=everything, act_dtype=torch.float32 if everything else torch.float64)
    if combo == 'state' or everything:
        eng.enable_state_rows(normalize=everything, dtype=torch.float64 if everything else None)


def attached_engine(shape, combo, batch=ATTACHED_BATCH, policies=True):
    eng = Engine(config_of(shape), batch, seed=11, first_env_index=2)
    if policies:
        eng.enable_policies()
    eng.reset()
    eng.reserve_rollout(ROLLOUT_STEPS, want_masks=True, search='none')
    attach(eng, combo)
    return eng


def issue_attached(eng, name, k, acts):
    """One call of ATTACHED_CALLS or REFUSED."""
    import ctypes
    from mate_amd._native import check
    if name in CALLS or name == 'observe':
        return issue(eng, name, k, acts)
    if name == 'reset':
        return eng.reset()
    if name == 'reset_masked':
        return eng.reset(env_mask=(torch.arange(eng.num_envs, device=eng.device) % 3 == 1))
    if name == 'step_selected':
        return eng.step_selected(auto_reset=k)
    if name == 'import_state':
        return eng.import_state(eng.export_state().roll(1, 0))
    if name == 'device_tick_on':
        return eng.device_tick(k)
    if name == 'device_tick_off':
        return eng.device_tick(False)
    if name == 'rollout_greedy_pipelined':
        return eng.rollout_greedy(ROLLOUT_STEPS, auto_reset='pipelined', want_masks=True)
    if name == 'step_selected_no_policies':
        return eng.step_selected(auto_reset=1)
    base, _, missing = name.rpartition('_no_')
    if base.startswith('rollout'):
        return getattr(eng, base)(ROLLOUT_STEPS, auto_reset=1, want_masks=False)
    io, _ = eng._io(want_masks=missing != 'masks')
    if missing == 'scalars':
        io.scalars_dev = None
    entry = getattr(eng.lib, 'mate_engine_' + base)
    args = (eng._h, ctypes.byref(io)) + ((None,) if base in ('step_greedy', 'step_selected') else ()) + (1, eng._stream())
    return check(entry(*args))


def digest(tensor):
    return hashlib.sha256(tensor.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def attached_row(eng, name, k, acts):
    """[status code, error text, {attached output: sha256 of its bytes behind the call}, sha256 of export_state()]"""
    code, text = 0, ''
    try:
        issue_attached(eng, name, k, acts)
    except EngineError as err:
        code, text = err.code, str(err)
    outputs = {key: digest(getattr(eng, key)) for key in ATTACHED_OUTPUTS if getattr(eng, key, None) is not None}
    return [code, text, outputs, digest(eng.export_state())]


def attached_record(shape):
    """{'columns': {combination: [attached_row of every call of ATTACHED_CALLS]}, 'refused': {id: attached_row of the refused call}}"""
    record = {'columns': {}, 'refused': {}}
    for combo in ATTACHED:
        eng = attached_engine(shape, combo)
        acts = actions_of(eng)
        record['columns'][combo] = [attached_row(eng, name, k, acts) for name, k in ATTACHED_CALLS]
        eng.close()
    for what, combo, before, name in REFUSED:
        eng = attached_engine(shape, combo, policies=name != 'step_selected_no_policies')
        acts = actions_of(eng)
        for earlier, k in before:
            issue_attached(eng, earlier, k, acts)
        record['refused'][what] = attached_row(eng, name, 1, acts)
        eng.close()
    return record


def attached_main(argv):
    """Every dispatch of the column set in order (the rocprofv3 --kernel-trace target); --record PATH: the record of every shape as JSON."""
    record_to = argv[argv.index('--record') + 1] if '--record' in argv else None
    shapes = [a for a in argv if a in ATTACHED_SHAPES] or ATTACHED_SHAPES
    record = {shape: attached_record(shape) for shape in shapes}
    for shape in shapes:
        for combo, rows in record[shape]['columns'].items():
            print(shape, combo, 'batch', ATTACHED_BATCH)
            for (name, k), row in zip(ATTACHED_CALLS, rows):
                print('  %-32s status %d %s' % ('%s/%d' % (name, k), row[0], row[1]))
        for what, row in record[shape]['refused'].items():
            print(shape, 'refused:', what, 'status', row[0], row[1])
    if record_to:
        with open(record_to, 'w') as fh:
            json.dump(record, fh, indent=0, sort_keys=True)
    print('done', sum(len(ATTACHED) * len(ATTACHED_CALLS) + len(REFUSED) for _ in shapes), 'calls')


# ---- the opponents column set
# Who plays each team of a call, which launches that takes and whose rows the step consumes (csrc/engine_host.h: plan_opponents), over the states the
# setters can reach: ONE engine per shape, reconfigured between states, direct calls only.
OPPONENT_SHAPES = ('MATE-4v8-9', '0v5-3', 'MATE-2v4-0 sub_wave')      # (no cameras: every camera selection is a no-op; set_sub_wave(True): the sub-wave one-launch step)
OPPONENT_BATCH = 8
TEAMS = ('camera', 'target')
# a team's plain selection, or the candidates of its mixture
TEAM_STATES = ('greedy', 'heuristic', ('greedy',), ('naive',), ('random', 'greedy'), ('heuristic', 'external'), ('greedy', 'heuristic', 'naive', 'random', 'external'))
CHANNEL_STATES = ((), ('camera',), ('target',), ('camera', 'target'))
CHANNEL = {'dropout_rate': 0.5, 'range_limit': 500.0}
OPPONENT_AUTO_RESETS = (1, 3)
OPPONENT_CALLS = [(name, k) for k in OPPONENT_AUTO_RESETS for name in ('step_greedy', 'step_versus_greedy_camera', 'step_versus_greedy_target', 'step_selected',
                                                                       'rollout_greedy', 'rollout_versus_greedy_camera', 'rollout_versus_greedy_target')]
# the setter refusals, each pair of calls in both orders: (id, the calls in order); a scenario starts from the plain Greedy state and a step_greedy follows it
_PAIRS = ([('channel / heuristic cameras', ('set_channel', 'camera'), ('set_opponent', 'camera', 'heuristic')),
           ('channel / heuristic camera candidate', ('set_channel', 'camera'), ('set_mixture', 'camera', ('heuristic', 'external')))] +
          [pair for team in TEAMS for pair in (('%s mixture / setter' % team, ('set_mixture', team, ('naive',)), ('set_opponent', team, 'heuristic')),
                                               ('%s observation mode / heuristic' % team, ('set_obs_mode', team, 'enhanced'), ('set_opponent', team, 'heuristic')),
                                               ('%s observation mode / heuristic candidate' % team, ('set_obs_mode', team, 'shared'), ('set_mixture', team, ('heuristic', 'external'))))])
REFUSALS = ([(what + ', in this order', (a, b)) for what, a, b in _PAIRS] + [(what + ', in the other order', (b, a)) for what, a, b in _PAIRS] +
            [('channel under a mixture that replaced the heuristic cameras', (('set_opponent', 'camera', 'heuristic'), ('set_mixture', 'camera', ('naive',)), ('set_channel', 'camera')))])


def opponent_states(shape):
    """(camera state, target state, channels) indices: the whole product (196 states of 14 calls: about a second on an MI355X)"""
    if shape.endswith('sub_wave'):      # the plain Greedy states only
        return [(0, 0, ch) for ch in range(len(CHANNEL_STATES))]
    return [(c, t, ch) for c in range(len(TEAM_STATES)) for t in range(len(TEAM_STATES)) for ch in range(len(CHANNEL_STATES))]


def opponent_engine(shape):
    name, _, sub = shape.partition(' ')
    eng = Engine(config_of(name), OPPONENT_BATCH, seed=11, first_env_index=2)
    if sub:
        eng.set_sub_wave(True)
    eng.enable_policies()
    eng.reset()
    eng.reserve_rollout(ROLLOUT_STEPS, want_masks=True, search='none')
    try:      # (refused without cameras: step_selected then reports it call by call)
        selection = torch.randint(0, 1 << eng.num_targets, (eng.num_envs, eng.num_cameras), generator=torch.Generator().manual_seed(5))
        eng.enable_selection(multi_selection=True, selection=selection.to(dtype=torch.int32, device=eng.device))
    except EngineError:
        pass
    return eng


def attempt(fn, *args, **kwargs):
    """[error code, error text] of one call"""
    try:
        fn(*args, **kwargs)
    except EngineError as err:
        return [err.code, str(err)]
    return [0, '']


def setter(eng, what, team, value=None):
    if what == 'set_channel':
        return attempt(eng.set_channel, team, **CHANNEL)
    if what == 'set_mixture':
        status = attempt(eng.set_opponent_mixture, team, value)
        if status[0] == 0 and 'external' in value and (eng.num_cameras, eng.num_targets)[TEAMS.index(team)] > 0:
            rows = eng.external_actions(team)      # the caller's rows: the same at every call
            rows.copy_(torch.linspace(-1.0, 1.0, rows.numel(), dtype=torch.float64).reshape(rows.shape) * (2.0 if team == 'camera' else 15.0))
        return status
    if what == 'set_obs_mode':
        return attempt(eng.set_obs_mode, **{team: value})
    assert what == 'set_opponent', what
    return attempt(eng.set_camera_opponent if team == 'camera' else eng.set_target_opponent, value)


def plain_greedy(eng):
    """Back to the state behind enable_policies(): no mixture, no channel, Greedy agents, plain rows."""
    for team in TEAMS:
        eng.clear_opponent_mixture(team)
        eng.clear_channel(team)
    eng.set_camera_opponent('greedy')
    eng.set_target_opponent('greedy')
    eng.set_obs_mode()


def configure(eng, state):
    """The state from the plain Greedy one: the opponents, then the channels.  Returns [error code, text] of every setter (a channel of the camera team
    is refused where the heuristic camera agent plays or could play it: the state then goes without)."""
    plain_greedy(eng)
    statuses = []
    for team, index in zip(TEAMS, state[:2]):
        what = TEAM_STATES[index]
        if what != 'greedy':
            statuses.append(setter(eng, 'set_mixture' if isinstance(what, tuple) else 'set_opponent', team, what))
    return statuses + [setter(eng, 'set_channel', team) for team in CHANNEL_STATES[state[2]]]


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def consumed(eng, name, acts):
    """Per team, which buffers policy_actions() equals bit for bit behind the call: the scripted_rows kinds, policy_actions(greedy_targets=True)
    ('greedy_targets'), the caller's joint action ('caller'), or ['none'] (['empty']: the team has nobody)."""
    got = eng.policy_actions(greedy_targets=True)
    out = []
    for team, name_of in enumerate(TEAMS):
        if got[team].numel() == 0:
            out.append(['empty'])
            continue
        sources = {}
        for kind in ('greedy', 'heuristic', 'external'):
            try:
                sources[kind] = eng.scripted_rows(name_of, kind)
            except EngineError:
                pass
        if team == 1:
            sources['greedy_targets'] = got[2]
        if name.endswith('_' + name_of):
            sources['caller'] = acts[team].to(torch.float64)
        elif name == 'step_selected' and team == 0 and getattr(eng, 'selection_actions', None) is not None:
            sources['caller'] = eng.selection_actions.to(torch.float64)
        out.append(sorted(kind for kind, rows in sources.items() if same_bytes(rows, got[team])) or ['none'])
    return out


def opponent_row(eng, name, k, acts, full=False):
    """[error code, error text, last_flow, consumed(), whether each team's channel_edges changed]; `full`: + the SHA-256 of every output, of
    policy_actions, of scripted_memory, of the channel edges and of export_state()"""
    edges = [matrix for team in TEAMS for matrix in eng.channel_edges(team)]
    before = [matrix.clone() for matrix in edges]
    code, text, out = 0, '', None
    try:
        out = issue_attached(eng, name, k, acts)
    except EngineError as err:
        code, text = err.code, str(err)
    changed = [not same_bytes(x, y) for x, y in zip(before, edges)]
    row = [code, text, eng.last_flow, consumed(eng, name, acts), [changed[0] or changed[1], changed[2] or changed[3]]]
    if full:
        memory = {}
        for team in TEAMS:
            try:
                memory[team] = {key: digest(value) for key, value in eng.scripted_memory(team).items()}
            except EngineError as err:
                memory[team] = err.code
        row.append({'outputs': [digest(t) for t in out or ()], 'policy_actions': [digest(t) for t in eng.policy_actions(greedy_targets=True)],
                    'scripted_memory': memory, 'channel_edges': [digest(matrix) for matrix in edges], 'state': digest(eng.export_state())})
    return row


def opponents_record(shape, full=False):
    """{'states': {state id: {'setters': configure(), 'calls': [opponent_row of every call of OPPONENT_CALLS]}},
        'refusals': {id: {'setters': [[error code, text] of each call of the scenario], 'step_greedy': opponent_row behind it}}}"""
    eng = opponent_engine(shape)
    acts = actions_of(eng)
    record = {'states': {}, 'refusals': {}}
    for state in opponent_states(shape):
        label = 'camera %s | target %s | channels %s' % ('+'.join(TEAM_STATES[state[0]]) if isinstance(TEAM_STATES[state[0]], tuple) else 'plain ' + TEAM_STATES[state[0]],
                                                         '+'.join(TEAM_STATES[state[1]]) if isinstance(TEAM_STATES[state[1]], tuple) else 'plain ' + TEAM_STATES[state[1]],
                                                         '+'.join(CHANNEL_STATES[state[2]]) or 'none')
        setters = configure(eng, state)
        record['states'][label] = {'setters': setters, 'calls': [opponent_row(eng, name, k, acts, full) for name, k in OPPONENT_CALLS]}
    if not shape.endswith('sub_wave'):
        for what, calls in REFUSALS:
            plain_greedy(eng)
            setters = [setter(eng, *call) for call in calls]
            record['refusals'][what] = {'setters': setters, 'step_greedy': opponent_row(eng, 'step_greedy', 1, acts, full)}
    plain_greedy(eng)
    torch.cuda.synchronize()
    eng.close()
    return record


def interned(obj, texts, grow=False):
    """`obj` with every error text replaced by '#<its index in texts>': the golden file holds each text once"""
    if isinstance(obj, str) and obj.startswith('mate_engine error'):
        if obj not in texts and grow:
            texts.append(obj)
        return '#%d' % texts.index(obj) if obj in texts else obj
    if isinstance(obj, (list, tuple)):
        return [interned(x, texts, grow) for x in obj]
    if isinstance(obj, dict):
        return {key: interned(value, texts, grow) for key, value in obj.items()}
    return obj


def one_entry_per_line(obj, depth):
    """JSON with the dictionaries of the first `depth` levels, and the lists right under the top, one entry per line"""
    compact = lambda value: json.dumps(value, separators=(',', ':'))
    if isinstance(obj, dict) and depth > 0:
        return '{\n' + ',\n'.join('%s:%s' % (compact(key), one_entry_per_line(value, depth - 1)) for key, value in obj.items()) + '\n}'
    if isinstance(obj, list) and depth == 3:
        return '[\n' + ',\n'.join(compact(value) for value in obj) + '\n]'
    return compact(obj)


def golden_of(record, commit):
    """tests/golden/opponent_flows.json from the record of every shape: the rows without the digests of a full record; each error text ('#<index>'),
    each distinct row (its index in 'rows') and each distinct list of a state's rows (its index in 'columns') once"""
    texts, rows, columns = [], [], []

    def row_index(row):
        row = interned(row[:5], texts, grow=True)
        if row not in rows:
            rows.append(row)
        return rows.index(row)
    def column_index(calls):
        column = [row_index(row) for row in calls]
        if column not in columns:
            columns.append(column)
        return columns.index(column)
    shapes = {shape: {'states': {label: {'setters': interned(state['setters'], texts, grow=True), 'calls': column_index(state['calls'])}
                                 for label, state in part['states'].items()},
                      'refusals': {what: {'setters': interned(scenario['setters'], texts, grow=True), 'step_greedy': row_index(scenario['step_greedy'])}
                                   for what, scenario in part['refusals'].items()}}
              for shape, part in record.items()}
    return {'recorded_with': 'python tools/launch_matrix.py opponents --golden PATH --commit %s: the build of that commit' % commit,
            'texts': texts, 'rows': rows, 'columns': columns, 'shapes': shapes}


def opponents_main(argv):
    """Every dispatch of the column set in order; --record PATH: the full record of every shape as JSON (two builds of the library: the same bytes);
    --golden PATH --commit ID: tests/golden/opponent_flows.json of this build, which is the build of commit ID."""
    record_to = argv[argv.index('--record') + 1] if '--record' in argv else None
    golden_to = argv[argv.index('--golden') + 1] if '--golden' in argv else None
    commit = argv[argv.index('--commit') + 1] if '--commit' in argv else 'unnamed'
    calls = 0
    record = {}
    for shape in OPPONENT_SHAPES:
        t0 = time.perf_counter()
        record[shape] = opponents_record(shape, full=record_to is not None)
        for label, state in record[shape]['states'].items():
            print(shape, '|', label, '| setters', [status[0] for status in state['setters']])
            for (name, k), row in zip(OPPONENT_CALLS, state['calls']):
                print('  %-34s status %d flow %d consumed %s edges %s %s' % ('%s/%d' % (name, k), row[0], row[2], row[3], row[4], row[1]))
                calls += 1
        for what, row in record[shape]['refusals'].items():
            print(shape, '| refusal:', what, '|', row['setters'], '| step_greedy:', row['step_greedy'][:5])
        print(shape, 'took %.1f s' % (time.perf_counter() - t0), flush=True)
    if record_to:
        with open(record_to, 'w') as fh:
            json.dump(record, fh, indent=0, sort_keys=True)
    if golden_to:
        with open(golden_to, 'w') as fh:
            fh.write(one_entry_per_line(golden_of(record, commit), 4) + '\n')
    print('done', calls, 'calls')


# ---- host cost per step with everything attached
def host_cost_main(argv):
    """One row per (call, form): step_versus_greedy (camera learner) and step_selected on MATE-4v8-9 with all three attached, direct (host
    microseconds per call of 512 enqueued back to back, and wall microseconds per step with the stream drained at the end) and as replays
    of a 16-step HIP graph under the device-resident step counter; five repeats each, every repeat printed."""
    batch = int(argv[0]) if argv else 4096
    eng = attached_engine('MATE-4v8-9', 'all', batch)
    import ctypes
    from mate_amd._native import check
    cam_io, keep = eng._io(cam_act=actions_of(eng)[0])
    sel_io, _ = eng._io()
    cam_ref, sel_ref = ctypes.byref(cam_io), ctypes.byref(sel_io)
    calls = {'step_versus_greedy': lambda: check(eng.lib.mate_engine_step_versus_greedy(eng._h, 0, cam_ref, None, 1, eng._stream())),
             'step_selected': lambda: check(eng.lib.mate_engine_step_selected(eng._h, sel_ref, None, 1, eng._stream()))}
    print('host-cost: MATE-4v8-9 x %d, state + reward (soft) + selection attached, auto_reset = 1' % batch)
    for name, call in calls.items():
        for _ in range(64):
            call()
        torch.cuda.synchronize()
        for rep in range(5):
            t0 = time.perf_counter()
            for _ in range(512):
                call()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            print('  %-20s direct rep %d: host %.2f us per call, %.2f us per step' % (name, rep, (t1 - t0) / 512 * 1e6, (t2 - t0) / 512 * 1e6), flush=True)
    eng.device_tick(1)
    for name, call in calls.items():
        call()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(16):
                call()
        for _ in range(8):
            graph.replay()
        torch.cuda.synchronize()
        for rep in range(5):
            t0 = time.perf_counter()
            for _ in range(32):
                graph.replay()
            torch.cuda.synchronize()
            print('  %-20s graph  rep %d: %.2f us per step' % (name, rep, (time.perf_counter() - t0) / 512 * 1e6), flush=True)
        del graph
    eng.device_tick(False)
    eng.close()


def main(argv):
    if argv[1:2] == ['attached']:
        return attached_main(argv[2:])
    if argv[1:2] == ['opponents']:
        return opponents_main(argv[2:])
    if argv[1:2] == ['host-cost']:
        return host_cost_main(argv[2:])
    shapes = argv[1:2] or SHAPES
    batches = [int(argv[2])] if len(argv) > 2 else [SMALL_BATCH, threshold_batch()]
    calls = 0
    for shape in shapes:
        for batch in batches:
            for dtype in DTYPES:
                for transform in (False, True):
                    for mode in MODES:
                        eng, in_use = make_engine(shape, batch, dtype, transform, mode)
                        print(column_id(shape, dtype, transform, mode), 'batch', batch, 'in_use', in_use, flush=True)
                        for call, values, _ in run_column(eng):
                            print('  %-32s flow %d sub_wave %d error %d' % (call, *values))
                            calls += 1
                        torch.cuda.synchronize()
                        eng.close()
    print('done', calls, 'calls')


if __name__ == '__main__':
    main(sys.argv)
