"""`Engine`: the batched step engine as torch tensors over the C ABI.

PyTorch is plumbing here (device memory, streams); all simulation work happens
in the HIP kernels behind ``include/mate_engine.h``.
"""
import ctypes
import os
import time
import warnings

import numpy as np
import torch

from mate_amd import _native, constants as consts, spaces
from mate_amd._native import MateChannel, MateConfig, MateMessageRows, MateFirstRows, MateFragmentRows, MateFrameFragments, MateLayout, MatePolicyTape, MateRewardRows, MateStepIO, check
from mate_amd.auxiliary_rewards import REWARD_REDUCTIONS, reward_coefficient_table, reward_term_keys      # noqa: F401 (this module's names too)
from mate_amd.config import scenario_tables

__all__ = ['Engine', 'EngineGroups', 'Stepper', 'export_layout', 'reward_coefficient_table', 'encode_selection', 'decode_selection',
           'SCALAR_NAMES', 'REWARD_REDUCTIONS', 'TARGET_AGENTS', 'CAMERA_AGENTS', 'SCRIPTED_AGENTS', 'mixture_table']

SCALAR_NAMES = ('camera_team_reward', 'target_team_reward', 'done', 'coverage_rate', 'real_coverage_rate',
                'mean_transport_rate', 'num_delivered_cargoes', 'normalized_target_team_reward')


def export_layout(Nc, Nt, No):
    """name -> (offset, shape) inside one row of `Engine.export_state()` ("state export")."""
    fields = [
        ('cam_x', (Nc,)), ('cam_y', (Nc,)), ('obs_x', (No,)), ('obs_y', (No,)), ('obs_radius', (No,)),
        ('tgt_capacity', (Nt,)), ('camera_obstacle_view_mask', (Nc, No)),
        ('cam_phi', (Nc,)), ('cam_theta', (Nc,)), ('tgt_x', (Nt,)), ('tgt_y', (Nt,)),
        ('tgt_colliding', (Nt,)), ('tgt_empty_bits', (Nt, 4)), ('tgt_goal_bits', (Nt, 4)), ('tgt_goals', (Nt,)),
        ('freights', (Nt,)), ('bounties', (Nt,)), ('target_steps', (Nt,)), ('tracked_steps', (Nt,)),
        ('remaining_cargoes', (4, 4)), ('awaiting_cargo_counts', (4,)), ('num_delivered_cargoes', ()),
        ('episode_reward', ()), ('delayed_episode_reward', ()), ('episode_step', ()), ('tick', ()), ('episode', ()),
        ('done', ()),
    ]
    layout, off = {}, 0
    for name, shape in fields:
        layout[name] = (off, shape)
        off += int(np.prod(shape)) if shape else 1
    return layout, off


CAMERA_AGENTS = ('greedy', 'heuristic')      # MATE_OPPONENT_* for the camera team (HeuristicCameraAgent: heuristic_tables.py, csrc/opponent_rows.hpp)
TARGET_AGENTS = ('greedy', 'heuristic')      # MATE_OPPONENT_* (include/mate_engine.h): the scripted agents that can play the target team

SCRIPTED_AGENTS = ('greedy', 'heuristic', 'naive', 'random', 'external')      # MATE_SCRIPTED_*: the candidates of an opponent mixture (csrc/scripted_rows.hpp)


def mixture_table(candidates, weights=None, random_frame_skip=20):
    """(kinds, weights) of an opponent mixture as mate_engine_set_opponent_mixture takes them, checked without a device: `candidates` a name
    of SCRIPTED_AGENTS, a sequence of names, or a dict name -> weight; `weights` (None: all 1) one non-negative finite number per candidate,
    not all zero (MixtureCameraAgent / MixtureTargetAgent, mate/agents/mixture.py:28-39).  ValueError otherwise."""
    import math
    if isinstance(candidates, str):
        candidates = [candidates]
    if isinstance(candidates, dict):
        if weights is not None:
            raise ValueError('a mixture given as a dict carries its weights: pass no `weights`')
        candidates, weights = list(candidates.keys()), list(candidates.values())
    candidates = list(candidates)
    if not candidates:
        raise ValueError('a mixture needs at least one candidate (clear_opponent_mixture removes one)')
    weights = [1.0] * len(candidates) if weights is None else [float(w) for w in weights]
    if len(weights) != len(candidates):
        raise ValueError(f'{len(candidates)} candidates but {len(weights)} weights')
    for name in candidates:
        if name not in SCRIPTED_AGENTS:
            raise ValueError(f'mixture candidates must be of {SCRIPTED_AGENTS}, got {name!r}')
    if len(set(candidates)) != len(candidates):
        raise ValueError(f'a mixture names every candidate once, got {candidates}')
    if any(not math.isfinite(w) or w < 0.0 for w in weights) or not any(w > 0.0 for w in weights):
        raise ValueError(f'mixture weights must be non-negative and finite with at least one positive value, got {weights}')
    if int(random_frame_skip) != random_frame_skip or random_frame_skip < 1:
        raise ValueError(f'random_frame_skip must be an integer >= 1, got {random_frame_skip!r}')
    return [SCRIPTED_AGENTS.index(name) for name in candidates], weights


NO_COMMUNICATION = ('both', 'camera', 'target', 'none')      # mate.NoCommunication's `team`, the reference's --no-communication


def channel_settings(range_limit=None, dropout_rate=0.0):
    """(limit, rate) of a communication channel as mate_engine_set_channel takes them, checked without a device: `range_limit` None, inf or
    negative for no limit (-1.0), never NaN; `dropout_rate` a finite number in [0, 1] (RandomMessageDropout's assertion).  ValueError otherwise."""
    import math
    limit = -1.0 if range_limit is None else float(range_limit)
    if math.isnan(limit):
        raise ValueError('the range limit of a channel is NaN (None, inf or a negative number: no limit)')
    if limit < 0.0 or math.isinf(limit):
        limit = -1.0
    rate = float(dropout_rate)
    if not math.isfinite(rate) or rate < 0.0 or rate > 1.0:
        raise ValueError(f'the dropout rate of a channel must be a float number between 0 and 1, got {dropout_rate!r}')
    return limit, rate


def channel_table(no_communication='none', message_dropout=0.0, communication_range=None):
    """Per team (camera, target): None, or the keywords of Engine.set_channel, from the three keywords the environments and the evaluation script
    take -- `no_communication` one of NO_COMMUNICATION, `message_dropout` a rate or (camera_rate, target_rate), `communication_range` a limit or
    (camera_limit, target_limit) (None: no limit).  Checked without a device; ValueError otherwise."""
    if no_communication not in NO_COMMUNICATION:
        raise ValueError(f'no_communication must be one of {NO_COMMUNICATION}, got {no_communication!r}')
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    rates, limits = pair(message_dropout), pair(communication_range)
    if len(rates) != 2 or len(limits) != 2:
        raise ValueError('message_dropout and communication_range take one value or a (camera, target) pair')
    table = []
    for team, name in enumerate(('camera', 'target')):
        limit, rate = channel_settings(limits[team], 0.0 if rates[team] is None else rates[team])
        disabled = no_communication in ('both', name)
        table.append(dict(disabled=disabled, range_limit=None if limit < 0 else limit, dropout_rate=rate) if disabled or limit >= 0 or rate > 0 else None)
    return table


def seat_mode_of(seat, shuffle_entities):
    """(mode, fixed seat, tape tensor) of Engine.enable_seat's `seat`: 'auto' is the reference's rule (single_team.py: index = num_teammates - 1,
    or np_random.randint(num_teammates) at every reset() under shuffle_entities); -1 as the fixed seat means n - 1."""
    if isinstance(seat, str):
        if seat not in ('auto', 'draw'):
            raise ValueError(f"seat = {seat!r}: 'auto', 'draw', an agent index or an [N] int32 tensor")
        return ('draw', 0, None) if seat == 'draw' or shuffle_entities else ('fixed', -1, None)
    if isinstance(seat, torch.Tensor):
        return 'tape', 0, seat
    if isinstance(seat, bool) or not isinstance(seat, (int, np.integer)) or seat < 0:
        raise ValueError(f"seat = {seat!r}: 'auto', 'draw', an agent index or an [N] int32 tensor")
    return 'fixed', int(seat), None


def encode_selection(selection, multi, num_envs, num_cameras, num_targets, device=None):
    """The reference's HierarchicalCamera action (examples/hrl/wrappers.py) -> the int32 words [N, Nc] mate_engine_enable_selection reads:
    multi-selection [N, Nc, Nt] of 0 / 1 -> bit t of the word (already packed [N, Nc] words pass through); single selection [N, Nc]
    indices in [0, Nt] (Nt: none) as they are.  Shape and dtype are checked, values are not.  Runs where `selection` lives."""
    selection = torch.as_tensor(selection, device=device)
    assert not selection.dtype.is_floating_point and not selection.dtype.is_complex, f'selections are integers (got {selection.dtype})'
    if multi and selection.dim() == 3:
        assert selection.shape == (num_envs, num_cameras, num_targets), tuple(selection.shape)
        weights = 1 << torch.arange(num_targets, device=selection.device, dtype=torch.int64)
        return ((selection != 0).to(torch.int64) * weights).sum(-1).to(torch.int32)
    assert selection.shape == (num_envs, num_cameras), tuple(selection.shape)
    return selection.to(torch.int32)


def decode_selection(words, multi, num_targets):
    """The words of encode_selection -> [..., Nt] bool, the targets the executor takes as selected (selection_kernel reads them the same
    way): bit t of a multi-selection word, bits beyond Nt ignored; the one-hot row of a single selection's index (the wrapper's
    index2onehot), all zero for Nt -- and for any index outside [0, Nt)."""
    words = torch.as_tensor(words).to(torch.int64)
    t = torch.arange(num_targets, device=words.device, dtype=torch.int64)
    if multi:
        return ((words[..., None] >> t) & 1).bool()
    return words[..., None] == t


FRAGMENT_REFUSED_KEYS = ('soft_coverage_score', 'normalized_goal_distance', 'sparse_delivery', 'is_colliding')


def fragment_coefficient_table(team, coefficients, reduction='none'):
    """reward_coefficient_table() for the shaped rows of a FrameSkip fragment (Engine.enable_fragment_rows): the same keys, order and
    assertions, but the four terms that need the state of every frame -- FRAGMENT_REFUSED_KEYS -- must be absent or 0; the
    fragment launch sees the scalar records and the masks only (the engine refuses them too, MATE_EINVAL)."""
    table = reward_coefficient_table(team, coefficients, reduction)
    for key in FRAGMENT_REFUSED_KEYS:
        assert not coefficients.get(key), (
            f'The term {key!r} needs the state of every frame and is not available in a fused fragment (got coefficient {coefficients[key]!r}); '
            f'use per-step launches with Engine.enable_reward_rows(accumulate=True) for it.')
    return table


class _EngineOwned:
    """Engine-owned device memory as a zero-copy tensor source (the tensor keeps `owner`, the Engine, alive)."""

    def __init__(self, owner, ptr, count, typestr):
        self.owner = owner
        self.__cuda_array_interface__ = {'shape': (count,), 'typestr': typestr, 'data': (ptr, False), 'version': 2}


def _team_code(team):
    """'camera' / 0 -> 0, 'target' / 1 -> 1."""
    code = {'camera': 0, 'target': 1}.get(team, team)
    assert code in (0, 1), f"team = {team!r}: 'camera' or 'target'"
    return code


class Engine:
    """N environments of one scenario on one GPU."""

    def __init__(self, config, num_envs, device=0, seed=0, first_env_index=0, obs_dtype=torch.float32):
        """`config` is a validated scenario mapping (mate_amd.config.read_config)."""
        self.lib = _native.load()
        self._block_switches = self._read_block_switches()
        self.config = config
        self.num_envs = int(num_envs)
        self.device_index = int(device)
        self.device = torch.device('cuda', self.device_index)
        self.obs_dtype = obs_dtype
        tables = scenario_tables(config)
        self._ranges = (tables['camera_ranges'], tables['target_ranges'], tables['obstacle_ranges'])      # (self._cfg points into them)
        self.num_cameras, self.num_targets, self.num_obstacles = tables['num_cameras'], tables['num_targets'], tables['num_obstacles']
        c = MateConfig()
        c.num_cameras, c.num_targets, c.num_obstacles = self.num_cameras, self.num_targets, self.num_obstacles
        c.max_episode_steps = int(config['max_episode_steps'])
        c.sparse_reward = int(config['reward_type'] == 'sparse')
        c.num_cargoes_per_target = int(config['num_cargoes_per_target'])
        c.shuffle_entities = int(bool(config['shuffle_entities']))
        c.targets_start_with_cargoes = int(bool(config['targets_start_with_cargoes']))
        c.high_capacity_target_split = float(config['high_capacity_target_split'])
        c.bounty_factor = float(config['bounty_factor'])
        c.transmittance = tables['transmittance']
        for key, value in tables['camera'].items():
            setattr(c, 'camera_' + key, value)
        c.target_step_size = float(config['target']['step_size'])
        c.target_sight_range = float(config['target']['sight_range'])
        c.obstacle_radius_range[0], c.obstacle_radius_range[1] = tables['obstacle_radius_range']
        dp = ctypes.POINTER(ctypes.c_double)
        c.camera_location_ranges, c.target_location_ranges, c.obstacle_location_ranges = (r.ctypes.data_as(dp) for r in self._ranges)
        c.obs_dtype = 1 if obs_dtype == torch.float64 else 0
        self._cfg = c
        handle = ctypes.c_void_p()
        check(self.lib.mate_engine_create(ctypes.byref(c), self.num_envs, self.device_index, int(seed), int(first_env_index), ctypes.byref(handle)))
        self._h = handle
        layout = MateLayout()
        check(self.lib.mate_engine_get_layout(self._h, ctypes.byref(layout)))
        self.layout = layout
        self.camera_obs_dim, self.target_obs_dim = layout.camera_obs_dim, layout.target_obs_dim
        self.specialised = bool(layout.specialised)   # shape-specialised step kernels in use (MATE_GENERIC=1 forces generic)
        self.export_fields, width = export_layout(self.num_cameras, self.num_targets, self.num_obstacles)
        assert width == layout.export_width, (width, layout.export_width)
        N, Nc, Nt = self.num_envs, self.num_cameras, self.num_targets
        with torch.cuda.device(self.device):
            self.camera_obs = torch.zeros((N, Nc, layout.camera_obs_dim), dtype=obs_dtype, device=self.device)
            self.target_obs = torch.zeros((N, Nt, layout.target_obs_dim), dtype=obs_dtype, device=self.device)
            self.scalars = torch.zeros((N, 8), dtype=torch.float32, device=self.device)
            self.masks = torch.zeros((N, layout.mask_words), dtype=torch.int32, device=self.device)
            # running sums over finished episodes (mate_amd.distributed.EpisodeStats.FIELDS): count, return, length, coverage, delivered
            self.episode_stats = torch.zeros(5, dtype=torch.float64, device=self.device)
        check(self.lib.mate_engine_set_episode_stats(self._h, ctypes.c_void_p(self.episode_stats.data_ptr())))
        self.state_dim = layout.state_dim
        self.target_agent = 'greedy'      # the scripted agent of the target team (set_target_opponent)
        self.camera_agent = 'greedy'      # ... and of the camera team (set_camera_opponent)
        self._camera_tables_installed = False
        self._camera_tape = (None, None)      # the tensors mate_engine_heuristic_camera_tape points at
        self.mixtures = [None, None]          # per team: None or {name: weight} of the installed opponent mixture (set_opponent_mixture)
        self._plain_agents = [None, None]     # ... and the plain selection it replaced
        self._scripted_tape = (None, None)    # the tensors mate_engine_scripted_tape points at
        self.channels = [None, None]          # per team: None or the settings of its communication channel (set_channel)
        self._channel_tape = (None, None, None)      # the tensors mate_engine_channel_tape points at
        self._clear_seat()
        self._clear_messages()
        self._message_tape = (None, None, None)      # the tensors mate_engine_message_tape points at
        self.camera_action_grid = self.target_action_grid = None      # (set_action_grids)
        self.outer_capacity = 0           # knots of Camera.boundary_outer once it is built (enable_outer_boundary)
        # (reserve_rollout) the buffers: None or {'steps', 'search', 'camera_obs', 'target_obs', 'scalars', 'masks', '_calls': _run_rollout's cache}
        self._rollout, self._block_search, self._reserve_t0 = None, None, None
        self.block_rates, self.store_form, self.reserve_seconds = [], 0, 0.0
        self._random_io = {}              # the cached argument blocks of step_random (_forget_calls)
        self._own_masks = False           # (keep_masks, enable_policies)
        self._policies = False            # (enable_policies)
        self.trace_duration, self.trace_teams = 0, ()      # (enable_communication_trace)
        self._staged = self._softcov = self._export_slices = None      # (stage_outputs, soft_coverage, state_dict_from)
        self._clear_state_rows()
        self._clear_reward_rows()
        self._clear_selection()
        self._clear_fragment_rows()
        self._clear_episode_records()
        self._clear_info_rows()

    # The detached value of every attached feature, written once: __init__ and the feature's disable_* both come here.
    def _clear_state_rows(self):
        self.state, self.state_normalized = None, False      # [N, state_dim] while state rows are attached (enable_state_rows)

    def _clear_reward_rows(self):
        # while reward rows are attached (enable_reward_rows): [N, Nc] / [N, Nt] shaped rewards, [N, Nc, 7] / [N, Nt, 10] f64 terms,
        # and the two coefficient tables on the device ({'camera': [7], 'target': [10]} f64)
        self.camera_reward_rows = self.target_reward_rows = self.camera_reward_terms = self.target_reward_terms = None
        self.reward_coefficients, self.reward_accumulate = None, False

    def _clear_selection(self):
        # while target selection is attached (enable_selection): the learner's selection [N, Nc] int32, the executor's joint action
        # [N, Nc, 2] (engine-owned), the metrics [N, Nc, 4] f64, the contributing frames [N] int32 and action_mask() [N, Nc, 2 Nt | Nt + 1] u8
        self.selection = self.selection_metrics = self.selection_frames = self.action_mask = None
        self._selection_actions_view = None      # (selection_actions: built at every read, never kept)
        self.multi_selection, self.selection_accumulate = None, False

    def _clear_fragment_rows(self):
        # while fragment rows are attached (enable_fragment_rows): what FrameSkip hands the learner per K-frame launch
        self.fragment_obs = self.fragment_rewards = self.fragment_done = self.fragment_frames = self.fragment_info = None
        self.fragment_shaped = self.fragment_team = None
        self._fragment_coefficients_view = None      # (fragment_coefficients: built at every read, never kept)
        self.fragment_frame_skip, self._fragment_masks = 0, False
        self.fragment_per_frame, self._frame_restarted = False, None      # (enable_fragment_rows(per_frame=True): built frame by frame behind step_versus_greedy)
        self._clear_first_rows()

    def _clear_first_rows(self):
        self.fragment_first_rows = self.fragment_first_scalars = self.fragment_final_obs = None      # (enable_fragment_rows(first_rows=True))

    def _clear_episode_records(self):
        # while episode records are attached (enable_episode_records): the ring [capacity, 16] f64, the count of records ever appended
        # [1] int64, the team's code, and how many of them episode_records() has handed out
        self.episode_ring = self.episode_count = self.episode_team = None
        self._episode_read = 0

    def _clear_seat(self):
        # while a learner's seat is enabled (enable_seat): the team's code, the mode, the seat's rows [N, D_team] (obs dtype), the seat of the
        # episode each row belongs to [N] int32, the seat whose action the last step_seated consumed [N] int32, the caller's tape (SEAT_TAPE)
        self.seat_team = self.seat_mode = self.seat_obs = self.seat_index = self.seat_acted = self._seat_tape = None

    def _clear_messages(self, team=None):
        # per team, while the learner's messages are enabled (enable_messages): the payload [N, n, M] / [N, n, n, M] and the inbox [N, n, n, M] (obs dtype),
        # the address matrix [N, n, n] uint8 or None (broadcast), the width M and whether the payload is per [sender][recipient]
        if team is None:
            self.message_payload, self.message_address, self.message_inbox = [None, None], [None, None], [None, None]
            self.message_width, self.message_pairwise = [0, 0], [False, False]
        else:
            self.message_payload[team] = self.message_address[team] = self.message_inbox[team] = None
            self.message_width[team], self.message_pairwise[team] = 0, False

    def _clear_info_rows(self):
        # while the training-information rows are attached (enable_info_rows): [N, Nc, 2] / [N, Nt, 9] / [N, 24] f64, None for an output that is off
        self.info_camera_rows = self.info_target_rows = self.info_cargo_rows = None

    def close(self):
        if getattr(self, '_h', None):
            self.lib.mate_engine_destroy(self._h)
            self._h = None
            self._clear_episode_records()
            self._selection_actions_view = self._fragment_coefficients_view = None      # (views of memory that is gone)

    __del__ = close

    # Zero-copy tensors over engine-owned memory keep the Engine alive (_EngineOwned).  The Engine must not keep THEM: that cycle would leave
    # its destruction -- mate_engine_destroy waits for the device and frees -- to the cyclic collector, which may run inside another
    # engine's stream capture.  So these two are (pointer, count, typestr, shape) records and the tensor is built at every read.
    def _owned_view(self, view):
        if view is None:
            return None
        ptr, count, typestr, shape = view
        return torch.as_tensor(_EngineOwned(self, ptr, count, typestr), device=self.device).view(shape)

    selection_actions = property(lambda self: self._owned_view(self._selection_actions_view))
    fragment_coefficients = property(lambda self: self._owned_view(self._fragment_coefficients_view))

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _bind_outputs(self, io, camera_obs, target_obs, scalars, masks=None):
        """The four output pointers of a MateStepIO, set here and nowhere else: no camera pointer without cameras, no mask pointer unless
        the call wants its masks (`masks` = None otherwise).  A tensor that is None leaves its pointer null."""
        io.camera_obs_dev = camera_obs.data_ptr() if self.num_cameras and camera_obs is not None else None
        io.target_obs_dev = target_obs.data_ptr() if target_obs is not None else None
        io.scalars_dev = scalars.data_ptr()
        io.masks_dev = masks.data_ptr() if masks is not None else None
        return io

    def _forget_calls(self):
        """Drop the cached argument blocks (step_random's, _run_rollout's): they hold raw pointers into the output tensors, so whatever
        re-homes or replaces an output tensor comes here."""
        self._random_io = {}
        if self._rollout is not None:
            self._rollout['_calls'] = {}

    def _env_mask(self, env_mask):
        """(uint8 pointer or None, the tensor to keep alive) of a reset's environment mask."""
        if env_mask is None:
            return None, None
        env_mask = env_mask.to(device=self.device, dtype=torch.uint8).contiguous()
        return ctypes.c_void_p(env_mask.data_ptr()), env_mask

    def _io(self, cam_act=None, tgt_act=None, tape_ct=None, tape_goal=None, want_masks=True):
        io = MateStepIO()
        keep = []
        if tgt_act is not None or cam_act is not None:
            # integer tensors are grid indices (set_action_grids): int32 [N, agents]; reals are [N, agents, 2].
            # One team alone = the caller's team of step_versus_greedy.
            ints = (torch.int32, torch.int64, torch.int16, torch.uint8)
            if self.num_cameras == 0:
                cam_act = None
            teams = [team for team in (('camera', cam_act, self.num_cameras, self.camera_action_grid),
                                       ('target', tgt_act, self.num_targets, self.target_action_grid)) if team[1] is not None]
            reals = [act.dtype for _, act, _, _ in teams if act.dtype not in ints]
            act_dtype = reals[0] if reals else torch.float64
            assert act_dtype in (torch.float32, torch.float64)
            io.act_dtype = 1 if act_dtype == torch.float64 else 0
            for name, act, agents, grid in teams:
                if act.dtype in ints:
                    assert grid is not None, f'call set_action_grids({name}_levels=...) first'
                    act = act.to(torch.int32).contiguous()
                    assert act.numel() == self.num_envs * agents and act.device == self.device
                    io.act_dtype |= 0x100 if name == 'camera' else 0x200
                else:
                    act = act.to(act_dtype).contiguous()
                    assert act.numel() == self.num_envs * agents * 2 and act.device == self.device
                setattr(io, name + '_actions_dev', act.data_ptr())
                keep.append(act)
        if tape_ct is not None and self.num_cameras:
            tape_ct = tape_ct.to(torch.float64).contiguous()
            assert tape_ct.numel() == self.num_envs * self.num_cameras * self.num_targets
            io.tape_camera_target_dev = tape_ct.data_ptr()
            keep.append(tape_ct)
        if tape_goal is not None:
            tape_goal = tape_goal.to(torch.float64).contiguous()
            assert tape_goal.numel() == self.num_envs * self.num_targets
            io.tape_goal_dev = tape_goal.data_ptr()
            keep.append(tape_goal)
        return self._bind_outputs(io, self.camera_obs, self.target_obs, self.scalars, self.masks if want_masks else None), keep

    # ---------------------------------------------------------------------- API
    def set_obs_transform(self, relative_coordinates=False, rescaled_observation=False):
        """Fuse RelativeCoordinates / RescaledObservation (the reference's observation wrappers) into the
        kernel's packer.  The affine map of the rescale comes from the observation-space bounds
        (mate_amd.constants), exactly as `rescale_observation` derives it."""
        nums = (self.num_cameras, self.num_targets, self.num_obstacles)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        if rescaled_observation:
            cs, cb = spaces.rescale_affine(consts.camera_observation_space_of(*nums))
            ts, tb = spaces.rescale_affine(consts.target_observation_space_of(*nums))
            check(self.lib.mate_engine_set_obs_transform(self._h, int(relative_coordinates), ptr(cs), ptr(cb), ptr(ts), ptr(tb)))
        else:
            check(self.lib.mate_engine_set_obs_transform(self._h, int(relative_coordinates), None, None, None, None))

    OBS_MODES = {None: 0, False: 0, 'none': 0, 'plain': 0, 'enhanced': 1, 'shared': 2}

    def set_obs_mode(self, camera='plain', target='plain'):
        """Per-team observation mode fused into the packer: 'plain', 'enhanced' (the reference's
        EnhancedObservation wrapper) or 'shared' (SharedFieldOfView)."""
        check(self.lib.mate_engine_set_obs_mode(self._h, self.OBS_MODES[camera], self.OBS_MODES[target]))

    def set_action_grids(self, camera_levels=None, target_levels=None):
        """Discrete joint actions (the reference's DiscreteCamera / DiscreteTarget wrappers,
        wrappers/discrete_action_spaces.py): actions passed as int32 indices into `levels**2` grids are decoded
        in the step kernel.  The normalised grids are computed here with the reference's own NumPy formulas
        and handed to the engine as tables."""
        cg = np.ascontiguousarray(spaces.camera_action_grid(camera_levels), dtype=np.float64) if camera_levels else None
        tg = np.ascontiguousarray(spaces.target_action_grid(target_levels), dtype=np.float64) if target_levels else None
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
        check(self.lib.mate_engine_set_action_grids(self._h, ptr(cg), 0 if cg is None else len(cg), ptr(tg), 0 if tg is None else len(tg)))
        self.camera_action_grid, self.target_action_grid = cg, tg

    def seed(self, seed):
        check(self.lib.mate_engine_seed(self._h, int(seed)))

    def reset(self, env_mask=None):
        io, keep = self._io()
        mask_ptr, env_mask = self._env_mask(env_mask)
        check(self.lib.mate_engine_reset(self._h, mask_ptr, ctypes.byref(io), self._stream()))
        return self.camera_obs, self.target_obs

    def reset_tape(self, tape, tape_ct=None, env_mask=None):
        """reset() with the random draws taken from `tape` ([N, L] uniforms in the reference's call order, see
        mate_engine_reset_tape) and the see-through draws of the first view from `tape_ct` ([N, Nc, Nt]).  Returns
        (camera_obs, target_obs, draws_used [N] int32)."""
        tape = tape.to(device=self.device, dtype=torch.float64).contiguous()
        assert tape.dim() == 2 and tape.shape[0] == self.num_envs
        io, keep = self._io(tape_ct=tape_ct)
        used = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        mask_ptr, env_mask = self._env_mask(env_mask)
        check(self.lib.mate_engine_reset_tape(self._h, mask_ptr, ctypes.byref(io), ctypes.c_void_p(tape.data_ptr()), int(tape.shape[1]),
                                              ctypes.c_void_p(used.data_ptr()), self._stream()))
        return self.camera_obs, self.target_obs, used

    def step(self, cam_act, tgt_act, tape_ct=None, tape_goal=None, auto_reset=False):
        io, keep = self._io(cam_act, tgt_act, tape_ct, tape_goal)
        check(self.lib.mate_engine_step(self._h, ctypes.byref(io), int(auto_reset), self._stream()))
        return self.camera_obs, self.target_obs, self.scalars

    def step_random(self, auto_reset=True, want_masks=False):
        # the argument structure of this call never changes: built once per (masks or not), the host cost per step
        # matters when the step kernel is a dozen microseconds
        ref = self._random_io.get(want_masks)
        if ref is None:
            io, _ = self._io(want_masks=want_masks)
            ref = self._random_io[want_masks] = (io, ctypes.byref(io))
        status = self.lib.mate_engine_step_random(self._h, ref[1], int(auto_reset), self._stream())
        if status != 0:
            check(status)
        return self.camera_obs, self.target_obs, self.scalars

    RESET_PIPELINED = -1     # MATE_RESET_PIPELINED (include/mate_engine.h)

    @classmethod
    def _auto_reset_code(cls, auto_reset):
        """'pipelined' -> MATE_RESET_PIPELINED; ('pipelined', m) -> -m: one restart launch (on the engine's side stream) behind every
        m-th rollout launch; everything else as it is."""
        if auto_reset == 'pipelined':
            return cls.RESET_PIPELINED
        if isinstance(auto_reset, tuple):
            if len(auto_reset) != 2 or auto_reset[0] != 'pipelined' or not 1 <= int(auto_reset[1]) <= 1 << 16:
                raise ValueError(f"auto_reset = {auto_reset!r}: ('pipelined', m) takes 1 <= m <= 65536")
            return -int(auto_reset[1])
        if int(auto_reset) < 0 and int(auto_reset) != cls.RESET_PIPELINED:      # (a typo such as -5 would silently defer restarts five launches)
            raise ValueError(f"auto_reset = {auto_reset!r}: negative values other than Engine.RESET_PIPELINED are spelt ('pipelined', m)")
        return int(auto_reset)

    def rollout_greedy(self, steps, auto_reset=True, want_masks=False):
        """`steps` fused (agents act, environment steps) iterations of the on-device Greedy policies (enable_policies()
        first).  Same rollout-shaped tensors as rollout_random.  auto_reset = 'pipelined' (Engine.RESET_PIPELINED): the reset of
        what a launch finishes runs on the engine's side stream under the next launch, restarted environments join the one after."""
        auto_reset = self._auto_reset_code(auto_reset)
        return self._run_rollout(self.lib.mate_engine_rollout_greedy, steps, auto_reset, want_masks)

    def rollout_versus_greedy(self, team, joint_action, steps, auto_reset=True, want_masks=False):
        """FrameSkip(frame_skip=steps) over MultiCamera / MultiTarget (examples/utils/wrappers.py:301-323 over
        mate/wrappers/single_team.py:245-264) in ONE launch: the caller's `team` repeats `joint_action` for `steps` frames while
        the on-device greedy opponents act anew on every frame.  Rollout-shaped tensors; the caller sums the reward rows."""
        team = _team_code(team)
        auto_reset = self._auto_reset_code(auto_reset)
        steps = int(steps)
        want_masks = want_masks or (self._fragment_masks and self.fragment_team == team)
        buf = self.reserve_rollout(steps, want_masks)
        io, keep = self._io(cam_act=joint_action if team == 0 else None, tgt_act=joint_action if team == 1 else None)
        self._bind_outputs(io, buf['camera_obs'], buf['target_obs'], buf['scalars'], buf['masks'] if want_masks else None)
        check(self.lib.mate_engine_rollout_versus_greedy(self._h, team, ctypes.byref(io), steps, int(auto_reset), self._stream()))
        return buf['camera_obs'][:steps], buf['target_obs'][:steps], buf['scalars'][:steps]

    def rollout_random(self, steps, auto_reset=True, want_masks=False):
        """`steps` fused steps under the on-device random policy.  Returns rollout-shaped tensors
        (camera_obs [T,N,Nc,Dc], target_obs [T,N,Nt,Dt], scalars [T,N,8]); scalars[..., 2] == 2 marks
        steps skipped because the episode had already ended inside this rollout."""
        return self._run_rollout(self.lib.mate_engine_rollout_random, steps, auto_reset, want_masks)

    # Host-side switches of the observation-block search (read ONCE, when the Engine is built; include/mate_engine.h lists them)
    @staticmethod
    def _read_block_switches():
        env = os.environ
        return {
            'plain': env.get('MATE_PLAIN_BLOCKS') == '1',
            # (0 or less: no search at all -- one block, unprobed)
            'candidates': max(1, int(env['MATE_BLOCK_CANDIDATES'])) if 'MATE_BLOCK_CANDIDATES' in env else None,
            # the deep search (candidates separated by 12 GB spacers, a transient footprint of up to 45 % of the free memory) is
            # OPT-IN: reserve_rollout(search='deep') -- bench.py asks for it -- or MATE_BLOCK_DEEP=1; by default a few candidates side
            # by side within 0.3 s
            'deep': env.get('MATE_BLOCK_DEEP', '0') != '0',
            'seconds': float(env['MATE_BLOCK_SECONDS']) if 'MATE_BLOCK_SECONDS' in env else None,
            'deep_gib': float(env.get('MATE_BLOCK_GIB', '96')),
            'store_form': env.get('MATE_STORE_FORM', 'auto'),
        }

    def _observation_block(self, shape, deep=False):
        """A zeroed [steps][N][...] observation block and the store rates [GB/s] of the candidates probed for it.  Blocks of
        64 MiB and more come from ``mate_engine_block_alloc`` (2 MiB physical chunks in a shuffled order): the fused rollouts
        store 10-25 % faster into them than into what hipMalloc / the caching allocator hands out (include/mate_engine.h).
        MATE_PLAIN_BLOCKS=1: torch.zeros."""
        sw = self._block_switches
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=self.obs_dtype).element_size()
        if nbytes < (64 << 20) or sw['plain']:
            return torch.zeros(shape, dtype=self.obs_dtype, device=self.device), []
        # Shuffled chunks make a slow block unlikely, not impossible (tools/store_vmm.hip): blocks of 128 MiB and more -- the ones
        # a launch is bounded by -- are the fastest of up to MATE_BLOCK_CANDIDATES (default 6) candidates in the kernels' own
        # store pattern, where the device has the memory to hold them side by side; the search ends at the first candidate
        # that is a class (28 %) faster than another.
        # `deep` (the target block, which decides a launch's store rate): the fast blocks of a device lie in ZONES of its memory, 20-35 GB
        # wide and at a different depth on every GPU (tools/depth_probe.py: forty 4.4 GB blocks allocated in a row and held -- five to
        # twelve consecutive ones fast, the rest slow).  The deep search walks through the memory in allocation order -- a
        # candidate, a 12 GB spacer that is not probed, a candidate ... -- until one is fast (5.35 TB/s, or 28 % above the
        # slowest seen: the classes lie at ~4.2, ~5.0 and 5.4-6.1).  Its transient footprint is bounded three ways: 45 % of what is
        # free (two ranks that share a GPU in a test must both fit), MATE_BLOCK_GIB (default 96) GiB in absolute terms, and
        # MATE_BLOCK_SECONDS (default 3) of wall time -- a learner whose model already holds most of the HBM gets a short search,
        # not an out-of-memory error.  The wall-time bound covers BOTH blocks of a reserve_rollout (the camera block's candidates
        # take what the target block's search left, at least one).  Everything but the winner is freed at the end
        # (mate_engine_block_free: the physical memory comes back, the address range stays reserved).
        row_bytes = nbytes // (shape[0] * shape[1])
        search = self._block_search or ('deep' if sw['deep'] else 'shallow')
        tries = (sw['candidates'] or (6 if search == 'deep' else 3)) if nbytes >= (128 << 20) and row_bytes % 16 == 0 and search != 'none' else 1
        free = torch.cuda.mem_get_info(self.device)[0]
        deep = deep and tries > 1 and search == 'deep'
        seconds = sw['seconds'] if sw['seconds'] is not None else (3.0 if search == 'deep' else 0.3)
        spacer_bytes = 12 << 30
        budget = min(0.45 * free, sw['deep_gib'] * (1 << 30))
        if deep and sw['candidates'] is None:      # (an explicit count bounds the deep search too)
            tries = max(tries, int(budget // (nbytes + spacer_bytes)))
        tries = max(1, min(tries, int(free // (2 * nbytes))))
        t0 = self._reserve_t0 or time.perf_counter()      # (reserve_rollout's start: one time budget for both blocks)
        best, rates, held, spacers = None, [], [], []
        for _ in range(tries):
            try:
                block = _native.ScatteredBlock(self.device_index, nbytes)
            except _native.EngineError as err:      # no virtual-memory management on this driver, or out of memory: plain memory works as well
                if best is None:
                    warnings.warn(f'mate_engine_block_alloc failed ({err}); the rollout block comes from torch.zeros')
                    return torch.zeros(shape, dtype=self.obs_dtype, device=self.device), rates
                break
            if tries == 1:
                best = (0.0, block)
                break
            rate = block.store_rate(shape[1], row_bytes, self._stream())
            rates.append(rate)
            held.append(block)          # (kept until the search ends: a freed candidate would be handed out again)
            if best is None or rate > best[0]:
                best = (rate, block)
            if len(rates) > 1 and best[0] >= 1.28 * min(rates):
                break
            if time.perf_counter() - t0 > seconds:
                break
            if deep:
                if rate >= (5350.0 if nbytes >= (1 << 30) else 5100.0):      # (a short block's probe is a short launch: its ramp weighs more)
                    break
                try:
                    spacers.append(_native.HeldMemory(self.device_index, spacer_bytes))      # (moves the allocation on; never mapped, never touched)
                except _native.EngineError:
                    break
        block = best[1]
        del held, best
        del spacers
        return block.tensor(self.obs_dtype, shape).zero_(), rates

    def reserve_rollout(self, steps, want_masks=False, search=None):
        """Allocate the rollout-shaped output buffers ([steps][N][...]) now, so that a later rollout of up to `steps`
        steps allocates nothing (a training loop or a timed region calls this once up front).  Rows a launch does not
        write -- the observation rows of an environment that had finished earlier in the launch -- keep whatever they
        held; its scalar rows say done = 2.  `Engine.reserve_seconds` says how long the last (re)allocation took, candidate
        search included; `Engine.block_rates` = [target block's candidates, camera block's candidates] in GB/s.
        `search`: where the observation blocks come from -- 'shallow' (default: the fastest of up to three candidates allocated
        side by side, at most 0.3 s), 'deep' (the walk through the device's memory described in _observation_block: seconds,
        and a transient footprint of up to 45 % of the free HBM -- for a process that owns the GPU, e.g. bench.py), 'none' (one
        block, unprobed).  Every candidate that loses keeps its address range reserved (mate_engine_block_free), bounded per
        process by MATE_BLOCK_DEAD_GIB."""
        steps = int(steps)
        if search not in (None, 'shallow', 'deep', 'none'):
            raise ValueError(f"reserve_rollout(search={search!r}): 'shallow', 'deep', 'none' or None (= the last explicit choice)")
        if search is not None:                       # an explicit choice stays for the (re)allocations that follow, the internal ones included
            self._block_search = search
        buf = self._rollout
        depth = {'none': 0, 'shallow': 1, 'deep': 2}
        if buf is not None and search is not None and depth[search] > depth.get(buf.get('search'), 0) and buf['steps'] >= steps:
            warnings.warn(f"reserve_rollout(search={search!r}): the rollout buffers exist (searched {buf.get('search')!r}); release them "      # (kept: the deeper search was not run)
                          '(Engine.close() or a longer reservation) to search again', RuntimeWarning, stacklevel=2)
        if buf is None or buf['steps'] < steps or (want_masks and buf['masks'] is None):     # a shorter rollout fills a prefix
            t0 = self._reserve_t0 = time.perf_counter()
            N, Nc, Nt, L = self.num_envs, self.num_cameras, self.num_targets, self.layout
            self._rollout = None
            with torch.cuda.device(self.device):
                target_block, target_rates = self._observation_block((steps, N, Nt, L.target_obs_dim), deep=True)      # (first: its search holds the most memory)
                camera_block, camera_rates = self._observation_block((steps, N, Nc, L.camera_obs_dim))
                buf = {
                    'steps': steps, 'search': self._block_search or ('deep' if self._block_switches['deep'] else 'shallow'),
                    'camera_obs': camera_block,
                    'target_obs': target_block,
                    'scalars': torch.zeros((steps, N, 8), dtype=torch.float32, device=self.device),
                    'masks': torch.zeros((steps, N, L.mask_words), dtype=torch.int32, device=self.device) if want_masks else None,
                }
            self._rollout = buf
            self._forget_calls()
            self.block_rates = [target_rates, camera_rates]
            # where even the best candidate takes the rows slowly the stores bound a launch, and the line-aligned form of the row
            # stores wins 3 %; elsewhere it costs 1.3-2 % (include/mate_engine.h).  MATE_STORE_FORM=0 / 1 forces a form.
            form = self._block_switches['store_form']
            shifted = form == '1' or (form == 'auto' and bool(target_rates) and max(target_rates) < 4800.0)
            self.store_form = int(shifted)
            check(self.lib.mate_engine_set_store_form(self._h, int(shifted)))
            torch.cuda.synchronize(self.device)
            self.reserve_seconds = time.perf_counter() - t0
            self._reserve_t0 = None
        return buf

    def _run_rollout(self, entry_point, steps, auto_reset, want_masks):
        steps = int(steps)
        buf = self.reserve_rollout(steps, want_masks)
        # the argument block and the returned views of a (launch length, masks) combination never change while the buffers
        # live: built once -- a 20-step launch lasts 0.18 ms, and this call is what the GPU waits for before it starts
        cache = buf['_calls']
        call = cache.get((steps, bool(want_masks)))
        if call is None:
            io = self._bind_outputs(MateStepIO(), buf['camera_obs'], buf['target_obs'], buf['scalars'], buf['masks'] if want_masks else None)
            call = cache[(steps, bool(want_masks))] = (io, ctypes.byref(io), (buf['camera_obs'][:steps], buf['target_obs'][:steps], buf['scalars'][:steps]))
        status = entry_point(self._h, call[1], steps, int(auto_reset), self._stream())
        if status != 0:
            check(status)
        return call[2]

    def device_tick(self, enable=True):
        """Keep the step counter on the device (mate_engine_device_tick): step()/step_random() launches with
        auto_reset = `enable` (True = 1: immediate; k > 1: batched, one reset launch per k steps) then carry identical
        arguments in every reset interval and can be captured in a HIP graph.  False / 0 gives the counter back."""
        check(self.lib.mate_engine_device_tick(self._h, int(enable), self._stream()))

    def make_stepper(self, cam_act, tgt_act, auto_reset=True, graph_steps=0, between=None, versus=None, frame_skip=1):
        """A replayable `for _ in range(n): between(); step((cam_act, tgt_act))` loop over caller-owned action tensors
        (see Stepper); versus = 'camera' / 'target': the caller plays that team only, the greedy agents the other;
        frame_skip = K > 1 on top of `versus`: every step is one K-frame launch (FrameSkip, the example trainers' flow).
        With graph_steps > 0 the constructor runs `auto_reset` REAL steps before it captures (Stepper.warmup_steps)."""
        return Stepper(self, cam_act, tgt_act, auto_reset, graph_steps, between, versus, frame_skip)

    def enable_policies(self, target_agent='greedy', camera_agent='greedy'):
        """Allocate the on-device policy state (call before the reset whose observations the agents act on).  `target_agent` /
        `camera_agent`: the scripted agent that plays that team where the engine plays it (set_target_opponent / set_camera_opponent)."""
        for name, value, known in (('target_agent', target_agent, TARGET_AGENTS), ('camera_agent', camera_agent, CAMERA_AGENTS)):
            if value not in known:
                raise ValueError(f"{name} must be one of {known}, got {value!r}")
        check(self.lib.mate_engine_policy_enable(self._h))
        self._policies = True
        self._own_masks = True            # (the engine's own copy of the mask words exists from here on: render)
        if target_agent != 'greedy' or self.target_agent != 'greedy':
            self.set_target_opponent(target_agent)
        if camera_agent != 'greedy' or self.camera_agent != 'greedy':
            self.set_camera_opponent(camera_agent)

    def _install_camera_tables(self):
        """The Heuristic camera agents' three tables (heuristic_tables.py), built and installed once per engine; a scenario without cameras needs none."""
        if self.num_cameras == 0 or self._camera_tables_installed:
            return
        from mate_amd.heuristic_tables import heuristic_camera_tables
        camera = scenario_tables(self.config)['camera']
        tables = heuristic_camera_tables(camera['max_sight_range'], camera['min_viewing_angle'])
        check(self.lib.mate_engine_heuristic_camera_tables(self._h, *(table.ctypes.data_as(ctypes.c_void_p) for table in tables)))
        self._camera_tables_installed = True

    def _check_tensor(self, what, value, dtype, shape, named=None):
        """None, or a contiguous `dtype` tensor of `shape` on the engine's device (`named`: the type's word in the message; default: its short name)."""
        if value is not None and (value.dtype != dtype or tuple(value.shape) != tuple(shape) or not value.is_contiguous() or value.device != self.device):
            raise ValueError(f"{what} must be a contiguous {named or str(dtype).split('.')[-1]} tensor of shape {tuple(shape)} on {self.device}")

    def set_camera_opponent(self, camera_agent):
        """'greedy' (GreedyCameraAgent, the default) or 'heuristic' (HeuristicCameraAgent, mate/agents/heuristic.py:17-287: a central
        controller scores 756 poses per camera against the sensed targets in range, tries 32 orders of greedy assignment and hands
        every camera its goal pose) as the camera team of step_greedy and step_versus_greedy('target')
        (mate_engine_set_camera_opponent).  Any call boundary; enable_policies first.  The first switch builds the three tables
        (heuristic_tables.py) and installs them.  While 'heuristic' those calls run the heuristic cameras' launch in front of the
        step, the fused rollouts against the engine's cameras and a non-plain camera observation mode are refused; a scenario
        without cameras is unaffected."""
        if camera_agent not in CAMERA_AGENTS:
            raise ValueError(f"camera_agent must be one of {CAMERA_AGENTS}, got {camera_agent!r}")
        if camera_agent == 'heuristic':
            self._install_camera_tables()
        check(self.lib.mate_engine_set_camera_opponent(self._h, CAMERA_AGENTS.index(camera_agent)))
        self.camera_agent = camera_agent

    def heuristic_camera_tape(self, permutations=None, record=None):
        """Recorded permutations for the heuristic cameras' controller ([N, 32, Nc] int8 on the device; None: Philox draws) and a
        tensor of that shape that receives the permutations every launch used (None: nothing is stored).  Both hold until replaced."""
        shape = (self.num_envs, 32, self.num_cameras)
        for name, value in (('permutations', permutations), ('record', record)):
            self._check_tensor(name, value, torch.int8, shape)
        check(self.lib.mate_engine_heuristic_camera_tape(self._h, None if permutations is None else ctypes.c_void_p(permutations.data_ptr()),
                                                         None if record is None else ctypes.c_void_p(record.data_ptr())))
        self._camera_tape = (permutations, record)

    def heuristic_camera_goals(self):
        """(goals [N, Nc, 2] f64 -- (orientation, viewing angle), NaN where a camera has none --, state indices [N, Nc] i32, -1 where
        none) of the heuristic cameras' last launch."""
        goals = torch.zeros((self.num_envs, self.num_cameras, 2), dtype=torch.float64, device=self.device)
        index = torch.zeros((self.num_envs, self.num_cameras), dtype=torch.int32, device=self.device)
        check(self.lib.mate_engine_heuristic_camera_goals(self._h, ctypes.c_void_p(goals.data_ptr()), ctypes.c_void_p(index.data_ptr()), self._stream()))
        return goals, index

    def set_target_opponent(self, target_agent):
        """'greedy' (GreedyTargetAgent, the default) or 'heuristic' (HeuristicTargetAgent, mate/agents/heuristic.py:290-337: the
        Greedy action plus a drift away from the nearest camera sector's incentre) as the target team of step_greedy,
        step_versus_greedy('camera') and step_selected (mate_engine_set_target_opponent).  Any call boundary; enable_policies first.
        While 'heuristic' those calls are three launches (agents, drift, step), the fused rollouts against the engine's targets and a
        non-plain target observation mode are refused."""
        if target_agent not in TARGET_AGENTS:
            raise ValueError(f"target_agent must be one of {TARGET_AGENTS}, got {target_agent!r}")
        check(self.lib.mate_engine_set_target_opponent(self._h, TARGET_AGENTS.index(target_agent)))
        self.target_agent = target_agent

    def set_opponent_mixture(self, team, candidates, weights=None, random_frame_skip=20):
        """A per-episode MIXTURE of scripted agents as `team` ('camera' / 'target') where the engine plays it (MixtureCameraAgent /
        MixtureTargetAgent, mate/agents/mixture.py): at the team's first acting call of every episode each environment draws ONE candidate
        for the whole team.  `candidates`: names of SCRIPTED_AGENTS (or a dict name -> weight) -- 'greedy', 'heuristic', 'naive'
        (mate/agents/naive.py), 'random' (mate/agents/random.py: an action held for `random_frame_skip` calls), 'external' (the rows the
        caller writes into external_actions(team) before every stepping call).  One more launch in front of the step of step_greedy,
        step_versus_greedy and step_selected (mate_engine_set_opponent_mixture); a single 'greedy' or 'heuristic' candidate is that plain
        selection.  enable_policies first.  While installed, set_*_opponent of the team is refused, and unless the mixture is
        {'greedy'} so are the fused rollouts that would play the team."""
        team = _team_code(team)
        kinds, weights = mixture_table(candidates, weights, random_frame_skip)
        names = [SCRIPTED_AGENTS[k] for k, w in zip(kinds, weights) if w > 0.0]
        if 'heuristic' in names and team == 0:
            self._install_camera_tables()
        check(self.lib.mate_engine_set_opponent_mixture(self._h, team, (ctypes.c_int32 * len(kinds))(*kinds), (ctypes.c_double * len(kinds))(*weights),
                                                        len(kinds), int(random_frame_skip)))
        if self.mixtures[team] is None:
            self._plain_agents[team] = self.camera_agent if team == 0 else self.target_agent
        self.mixtures[team] = {SCRIPTED_AGENTS[k]: w for k, w in zip(kinds, weights) if w > 0.0}
        plain = 'heuristic' if 'heuristic' in names else 'greedy'      # (the Heuristic machinery of the team is on where a candidate needs it)
        setattr(self, ('camera_agent', 'target_agent')[team], plain)

    def clear_opponent_mixture(self, team):
        """Remove the team's mixture: the plain selection it replaced plays again (its Greedy agents reset at their next acting call)."""
        team = _team_code(team)
        check(self.lib.mate_engine_set_opponent_mixture(self._h, team, None, None, 0, 20))
        if self.mixtures[team] is not None:
            setattr(self, ('camera_agent', 'target_agent')[team], self._plain_agents[team])
        self.mixtures[team] = None

    def _scripted_shapes(self):
        N, Nc, Nt = self.num_envs, self.num_cameras, self.num_targets
        return (('camera_u', (N, Nc, 2), torch.float64), ('target_u', (N, Nt, 3), torch.float64), ('target_reset', (N, Nt, 4), torch.float64),
                ('choice', (2, N), torch.int32))

    def scripted_record(self):
        """A fresh record for scripted_tape(record=...): dict of device tensors of the tape's shapes."""
        return {name: torch.zeros(shape, dtype=dtype, device=self.device) for name, shape, dtype in self._scripted_shapes()}

    def scripted_tape(self, tape=None, record=None):
        """Recorded draws for the mixtures' launch and a record of the draws it used (mate_engine_scripted_tape): dicts of contiguous device
        tensors camera_u [N, Nc, 2], target_u [N, Nt, 3], target_reset [N, Nt, 4] f64 and choice [2, N] int32 (names of SCRIPTED_AGENTS by
        index, -1: draw).  A member the tape lacks is drawn (Philox); the record reads NaN where nothing was drawn.  Both hold until replaced."""
        pointers = []
        for which, given in (('tape', tape), ('record', record)):
            for name, shape, dtype in self._scripted_shapes():
                value = None if given is None else given.get(name)
                self._check_tensor(f'{which}[{name!r}]', value, dtype, shape, named=str(dtype))
                pointers.append(None if value is None else ctypes.c_void_p(value.data_ptr()))
        check(self.lib.mate_engine_scripted_tape(self._h, *pointers))
        self._scripted_tape = (tape, record)

    def scripted_memory(self, team):
        """The team's memory of the mixtures' launch as a dict of device tensors: choice [N] (index into SCRIPTED_AGENTS, -1 before the first
        draw), prev_action [N, n, 2] and counter [N] (the Random agents'), and for the targets goal, inc [N, Nt] and prev_noise [N, Nt, 2]
        (the Naive agents')."""
        team = _team_code(team)
        N, n = self.num_envs, (self.num_cameras, self.num_targets)[team]
        out = {'choice': torch.zeros(N, dtype=torch.int32, device=self.device), 'counter': torch.zeros(N, dtype=torch.int32, device=self.device),
               'prev_action': torch.zeros((N, n, 2), dtype=torch.float64, device=self.device)}
        if team == 1:
            out.update(goal=torch.zeros((N, n), dtype=torch.int32, device=self.device), inc=torch.zeros((N, n), dtype=torch.int32, device=self.device),
                       prev_noise=torch.zeros((N, n, 2), dtype=torch.float64, device=self.device))
        ptr = lambda name: ctypes.c_void_p(out[name].data_ptr()) if name in out else None
        check(self.lib.mate_engine_scripted_memory(self._h, team, ptr('choice'), ptr('goal'), ptr('inc'), ptr('prev_noise'), ptr('prev_action'), ptr('counter'),
                                                   self._stream()))
        return out

    def external_actions(self, team):
        """The engine-owned [N, n, 2] f64 tensor of the 'external' candidate of the team's mixture: fill it, for every environment, before each
        stepping call; the environments that drew 'external' play its rows."""
        team = _team_code(team)
        n = (self.num_cameras, self.num_targets)[team]
        ptr = ctypes.c_void_p()
        check(self.lib.mate_engine_scripted_external(self._h, team, ctypes.byref(ptr)))
        count = self.num_envs * n * 2
        return torch.as_tensor(_EngineOwned(self, ptr.value, count, '<f8'), device=self.device).view(self.num_envs, n, 2)

    def scripted_rows(self, team, kind):
        """One source of the team's final rows as the mixtures' last launch read it ([N, n, 2] f64): kind 'greedy', 'heuristic' or 'external'."""
        team = _team_code(team)
        n = (self.num_cameras, self.num_targets)[team]
        rows = torch.zeros((self.num_envs, n, 2), dtype=torch.float64, device=self.device)
        check(self.lib.mate_engine_scripted_rows(self._h, team, SCRIPTED_AGENTS.index(kind), ctypes.c_void_p(rows.data_ptr()), self._stream()))
        return rows

    # ------------------------------------------------------------------ communication channels (mate/wrappers/: NoCommunication, RandomMessageDropout, RestrictedCommunicationRange, MessageFilter)
    def set_channel(self, team, *, disabled=False, range_limit=None, dropout_rate=0.0, mask=None):
        """A communication channel for `team` ('camera' / 'target'): per step and per message sender -> recipient of the team's Greedy agents
        (and of the Heuristic targets, which inherit the Greedy targets' exchange) the message arrives only where the team is not `disabled`
        (NoCommunication), the two are at most `range_limit` apart (RestrictedCommunicationRange; None / inf / negative: no limit), the
        pair's binomial(1, dropout_rate) draws 0 (RandomMessageDropout) and `mask` ([N, n, n] uint8 on the device, [sender][recipient],
        read at every launch; None: all ones -- a MessageFilter with any function) is non-zero.  enable_policies first; any call boundary.
        While set for a team whose talking agents act, step_greedy / step_versus_greedy / step_selected take the two-launch form and the
        fused rollouts that would play the team are refused; a channel of the caller's own team or of Naive / Random agents is inert.
        Refused for a camera team the Heuristic agent plays (mate_engine_set_channel)."""
        team = _team_code(team)
        limit, rate = channel_settings(range_limit, dropout_rate)
        n = (self.num_cameras, self.num_targets)[team]
        self._check_tensor('mask', mask, torch.uint8, (self.num_envs, n, n))
        cfg = MateChannel(int(bool(disabled)), limit, rate, None if mask is None else mask.data_ptr())
        check(self.lib.mate_engine_set_channel(self._h, team, ctypes.byref(cfg)))
        self.channels[team] = {'disabled': bool(disabled), 'range_limit': None if limit < 0 else limit, 'dropout_rate': rate, 'mask': mask}

    def clear_channel(self, team):
        """Remove the team's channel: every message arrives again."""
        team = _team_code(team)
        check(self.lib.mate_engine_set_channel(self._h, team, None))
        self.channels[team] = None

    def channel_tape(self, camera_u=None, target_u=None, record=False):
        """Recorded dropout uniforms for the channels ([N, n, n] f64 device tensors, [sender][recipient]; None: Philox) and -- `record` -- two
        tensors of those shapes that receive the uniform every verdict used, NaN where none was drawn (mate_engine_channel_tape).  All hold
        until replaced.  Returns (record_camera_u, record_target_u), or None."""
        N, Nc, Nt = self.num_envs, self.num_cameras, self.num_targets
        for name, value, n in (('camera_u', camera_u, Nc), ('target_u', target_u, Nt)):
            self._check_tensor(name, value, torch.float64, (N, n, n))
        records = None
        if record:
            records = tuple(torch.full((N, n, n), float('nan'), dtype=torch.float64, device=self.device) for n in (Nc, Nt))
        ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        check(self.lib.mate_engine_channel_tape(self._h, ptr(camera_u), ptr(target_u), *(ptr(r) for r in (records or (None, None)))))
        self._channel_tape = (camera_u, target_u, records)
        return records

    def channel_edges(self, team):
        """(sent, delivered): zero-copy [N, n, n] int8 views, [sender][recipient], of the team's engine-owned edge matrices as the last
        agents' launch with a channel left them -- what the agents handed to the channel, and what arrived (the reference's
        camera_communication_edges / target_communication_edges)."""
        team = _team_code(team)
        n = (self.num_cameras, self.num_targets)[team]
        sent, delivered = ctypes.c_void_p(), ctypes.c_void_p()
        check(self.lib.mate_engine_channel_edges(self._h, team, ctypes.byref(sent), ctypes.byref(delivered)))
        count = self.num_envs * n * n
        if count == 0:
            return tuple(torch.zeros((self.num_envs, n, n), dtype=torch.int8, device=self.device) for _ in range(2))
        return tuple(torch.as_tensor(_EngineOwned(self, p.value, count, '|i1'), device=self.device).view(self.num_envs, n, n) for p in (sent, delivered))

    def channel_active(self, team_caller=None):
        """Whether a channel is set for a team the engine plays in a call where `team_caller` (None: neither) is the caller's."""
        caller = None if team_caller is None else _team_code(team_caller)
        return any(self.channels[t] is not None and t != caller for t in (0, 1))

    # ------------------------------------------------------------------ a learner seat among on-device teammates (mate/wrappers/single_team.py: SingleCamera / SingleTarget)
    SEAT_MODES = ('fixed', 'draw', 'tape')

    def enable_seat(self, team, seat='auto'):
        """The learner plays ONE agent of `team` ('camera' / 'target'), the seat; its n - 1 teammates are the team's on-device Greedy agents with
        their true indices, the opposing team is what set_*_opponent / set_opponent_mixture make of it.  `seat`: 'auto' -- the reference's rule:
        the constant n - 1 when the config's shuffle_entities is off, drawn anew per episode when it is on; 'draw'; an int; or an [N] int32
        device tensor read at every launch (a value outside [0, n) falls back to the draw).  enable_policies first.  Enabling, changing or
        disabling the seat resets that team's Greedy agents at their next acting call.  Returns (seat_obs [N, D_team], seat_index [N], seat_acted [N])."""
        team = _team_code(team)
        n, D = ((self.num_cameras, self.camera_obs_dim), (self.num_targets, self.target_obs_dim))[team]
        mode, fixed, tape = seat_mode_of(seat, bool(self.config['shuffle_entities']))
        if tape is not None:
            self._check_tensor('seat', tape, torch.int32, (self.num_envs,))
        if self.seat_obs is None or self.seat_team != team:
            with torch.cuda.device(self.device):
                outputs = (torch.zeros((self.num_envs, D), dtype=self.obs_dtype, device=self.device),
                           torch.zeros(self.num_envs, dtype=torch.int32, device=self.device), torch.zeros(self.num_envs, dtype=torch.int32, device=self.device))
        else:
            outputs = (self.seat_obs, self.seat_index, self.seat_acted)
        check(self.lib.mate_engine_enable_seat(self._h, team, self.SEAT_MODES.index(mode), fixed, None if tape is None else ctypes.c_void_p(tape.data_ptr()),
                                               *(ctypes.c_void_p(t.data_ptr()) for t in outputs)))
        self.seat_team, self.seat_mode, self._seat_tape = team, mode, tape
        self.seat_obs, self.seat_index, self.seat_acted = outputs
        return outputs

    def disable_seat(self):
        """Remove the seat: the team's Greedy agents (all n of them again) start afresh at their next acting call."""
        check(self.lib.mate_engine_enable_seat(self._h, 0, 0, 0, None, None, None, None))
        self._clear_seat()

    def _seat_io(self, action, tape_ct=None, tape_goal=None):
        """The argument block of a seat call: the seat's action ([N, 2] reals or [N] grid indices) in the seat team's action pointer."""
        assert self.seat_obs is not None, 'Engine.enable_seat() first'
        io, keep = self._io(tape_ct=tape_ct, tape_goal=tape_goal)
        if action is not None:
            name, grid = (('camera', self.camera_action_grid), ('target', self.target_action_grid))[self.seat_team]
            if action.dtype in (torch.int32, torch.int64, torch.int16, torch.uint8):
                assert grid is not None, f'call set_action_grids({name}_levels=...) first'
                action = action.to(torch.int32).contiguous()
                assert action.numel() == self.num_envs and action.device == self.device
                io.act_dtype = 0x100 if name == 'camera' else 0x200
            else:
                assert action.dtype in (torch.float32, torch.float64), 'the seat\'s action is f32 / f64 pairs or integer grid indices'
                action = action.contiguous()
                assert action.numel() == self.num_envs * 2 and action.device == self.device
                io.act_dtype = 1 if action.dtype == torch.float64 else 0
            setattr(io, name + '_actions_dev', action.data_ptr())
            keep.append(action)
        return io, keep

    def step_seated(self, action, policy_tape=None, tape_ct=None, tape_goal=None, auto_reset=True):
        """One step of SingleCamera / SingleTarget: `action` is the seat's ([N, 2] reals or [N] grid indices), the teammates and the opponents
        act on the device.  `policy_tape` keeps its full shapes (the seat's entries are ignored).  Returns (seat_obs, scalars): the seat's row
        of the new observations -- after an immediate restart the new episode's seat's -- and the team-level scalar rows; seat_index /
        seat_acted say whose row that is and whose action the step consumed; camera_obs / target_obs hold the full rows as ever."""
        io, keep = self._seat_io(action, tape_ct, tape_goal)
        check(self.lib.mate_engine_step_seated(self._h, ctypes.byref(io), self._policy_tape(policy_tape, keep), int(auto_reset), self._stream()))
        return self.seat_obs, self.scalars

    def seat_rows(self):
        """The gather on demand (behind reset()): every environment's seat row of the engine's observation tensors into seat_obs, its seat
        into seat_index.  Returns (seat_obs, seat_index)."""
        io, keep = self._seat_io(None)
        check(self.lib.mate_engine_seat_rows(self._h, ctypes.byref(io), self._stream()))
        return self.seat_obs, self.seat_index

    # ------------------------------------------------------------------ the learner's own messages through the team's channel (mate/environment.py: send_messages / receive_messages, the communication edges of `info`)
    def enable_messages(self, team, width, pairwise=False, addressed=False):
        """Fixed-width messages of `team`'s learner agents on the device: `width` numbers of the observation dtype per message, routed sender ->
        recipient by route_messages() under the team's channel (set_channel; none: everything arrives).  Returns (payload, address, inbox): the
        payload tensor the learner writes, [N, n, width] (one content per sender) or, `pairwise`, [N, n, n, width] ([sender][recipient]); with
        `addressed` the [N, n, n] uint8 address matrix ([sender][recipient], non-zero = send; starts all ones), else None: every sender broadcasts
        to every slot of its team, its own included; the inbox [N, n, n, width], [recipient][sender], zeros where nothing was sent or arrived.
        Needs no enable_policies.  Enabling again with the same shapes keeps the tensors and starts the counts afresh."""
        team = _team_code(team)
        n, N, width = (self.num_cameras, self.num_targets)[team], self.num_envs, int(width)
        if n == 0 or width < 1:
            raise ValueError(f'enable_messages: a team with agents and width >= 1 (got {n} agents, width = {width})')
        shape = (N, n, n, width) if pairwise else (N, n, width)
        payload, address, inbox = self.message_payload[team], self.message_address[team], self.message_inbox[team]
        with torch.cuda.device(self.device):
            if payload is None or tuple(payload.shape) != shape:
                payload = torch.zeros(shape, dtype=self.obs_dtype, device=self.device)
            if inbox is None or tuple(inbox.shape) != (N, n, n, width):
                inbox = torch.zeros((N, n, n, width), dtype=self.obs_dtype, device=self.device)
            if not addressed:
                address = None
            elif address is None:
                address = torch.ones((N, n, n), dtype=torch.uint8, device=self.device)
        cfg = MateMessageRows(width, int(bool(pairwise)), payload.data_ptr(), None if address is None else address.data_ptr(), inbox.data_ptr())
        check(self.lib.mate_engine_enable_messages(self._h, team, ctypes.byref(cfg)))
        self.message_payload[team], self.message_address[team], self.message_inbox[team] = payload, address, inbox
        self.message_width[team], self.message_pairwise[team] = width, bool(pairwise)
        return payload, address, inbox

    def disable_messages(self, team=None):
        """Detach the messages of `team` (None: of both teams)."""
        for t in ((0, 1) if team is None else (_team_code(team),)):
            check(self.lib.mate_engine_enable_messages(self._h, t, None))
            self._clear_messages(t)

    def route_messages(self, teams=None, round=0):
        """One launch: the payloads of `teams` ('camera' / 'target', a pair of them, None: every enabled team) go through their channels into the
        inboxes, the edge counts follow (message_edges).  `round` (0..15) keys the dropout draws: route twice between two steps with two rounds.
        Identical arguments at every call: replayable inside a Stepper graph (make_stepper(..., between=...))."""
        if teams is None:
            codes = [t for t in (0, 1) if self.message_inbox[t] is not None]
        else:
            codes = [_team_code(t) for t in (teams if isinstance(teams, (list, tuple)) else (teams,))]
        status = self.lib.mate_engine_route_messages(self._h, sum(1 << t for t in set(codes)), int(round), self._stream())
        if status != 0:
            check(status)
        return tuple(self.message_inbox[t] for t in codes)

    MESSAGE_EDGES = ('sent', 'delivered', 'step_edges', 'total_edges', 'agent_edges')

    def message_edges(self, team):
        """{'sent', 'delivered': int8 [N, n, n] of the last routing call; 'step_edges': int32 [N, n, n], the deliveries since the last step (the
        reference's *_communication_edges); 'total_edges': int32 [N, n, n], the episode's earlier steps (the reference's
        *_total_communication_edges as its last step left them); 'agent_edges': int32 [N, n, 2], out_ / in_communication_edges of `info`}:
        zero-copy views of the team's engine-owned matrices, [sender][recipient]."""
        team = _team_code(team)
        n, N = (self.num_cameras, self.num_targets)[team], self.num_envs
        pointers = [ctypes.c_void_p() for _ in self.MESSAGE_EDGES]
        check(self.lib.mate_engine_message_edges(self._h, team, *(ctypes.byref(p) for p in pointers)))
        shapes = [(N, n, n)] * 4 + [(N, n, 2)]
        typestrs = ['|i1', '|i1', '<i4', '<i4', '<i4']
        return {name: torch.as_tensor(_EngineOwned(self, p.value, int(np.prod(shape)), typestr), device=self.device).view(shape)
                for name, p, shape, typestr in zip(self.MESSAGE_EDGES, pointers, shapes, typestrs)}

    def message_tape(self, camera_u=None, target_u=None, record=False):
        """Recorded dropout uniforms for the routed messages ([N, n, n] f64 device tensors, [sender][recipient]; None: Philox) and -- `record` --
        two tensors of those shapes that receive the uniform every verdict used, NaN where none was drawn (mate_engine_message_tape).  All hold
        until replaced.  Returns (record_camera_u, record_target_u), or None."""
        N, Nc, Nt = self.num_envs, self.num_cameras, self.num_targets
        for name, value, n in (('camera_u', camera_u, Nc), ('target_u', target_u, Nt)):
            self._check_tensor(name, value, torch.float64, (N, n, n))
        records = None
        if record:
            records = tuple(torch.full((N, n, n), float('nan'), dtype=torch.float64, device=self.device) for n in (Nc, Nt))
        ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        check(self.lib.mate_engine_message_tape(self._h, ptr(camera_u), ptr(target_u), *(ptr(r) for r in (records or (None, None)))))
        self._message_tape = (camera_u, target_u, records)
        return records

    def _policy_tape(self, policy_tape, keep):
        if policy_tape is None:
            return None
        tape = MatePolicyTape()
        for name, dtype in (('camera_resample_u', torch.float64), ('camera_sample_u', torch.float64), ('camera_delay', torch.int32),
                            ('target_choice_u', torch.float64), ('target_resample_u', torch.float64), ('target_sample_u', torch.float64),
                            ('target_reset_sample_u', torch.float64)):
            value = policy_tape.get(name)
            if value is not None:
                value = value.to(device=self.device, dtype=dtype).contiguous()
                keep.append(value)
                setattr(tape, name + '_dev', value.data_ptr())
        return ctypes.byref(tape)

    def step_greedy(self, policy_tape=None, tape_ct=None, tape_goal=None, auto_reset=True):
        """One step with GreedyCameraAgent vs GreedyTargetAgent computed on the device.  `policy_tape`:
        dict of recorded agent draws (tensors) for parity runs.  Returns (camera_obs, target_obs, scalars)."""
        io, keep = self._io(tape_ct=tape_ct, tape_goal=tape_goal)
        check(self.lib.mate_engine_step_greedy(self._h, ctypes.byref(io), self._policy_tape(policy_tape, keep), int(auto_reset), self._stream()))
        return self.camera_obs, self.target_obs, self.scalars

    def step_versus_greedy(self, team, joint_action, policy_tape=None, tape_ct=None, tape_goal=None, auto_reset=True):
        """MultiCamera (team = 'camera' / 0) or MultiTarget (team = 'target' / 1), mate/wrappers/single_team.py:245-264:
        `joint_action` is the caller's team ([N, agents, 2] reals or [N, agents] grid indices), the opponents are the
        on-device greedy agents.  Returns (camera_obs, target_obs, scalars)."""
        team = _team_code(team)
        io, keep = self._io(cam_act=joint_action if team == 0 else None, tgt_act=joint_action if team == 1 else None,
                            tape_ct=tape_ct, tape_goal=tape_goal)
        check(self.lib.mate_engine_step_versus_greedy(self._h, team, ctypes.byref(io), self._policy_tape(policy_tape, keep),
                                                      int(auto_reset), self._stream()))
        return self.camera_obs, self.target_obs, self.scalars

    def policy_actions(self, greedy_targets=False):
        """(camera_actions [N,Nc,2], target_actions [N,Nt,2]) f64: the joint actions of the last step_greedy, as the step consumed
        them -- with the heuristic target opponent the final target actions -- and until the next stepping call: a setter in between
        (set_*_opponent, set_opponent_mixture, set_channel) does not change what is reported.  greedy_targets=True: a third tensor, the Greedy
        target agents' joint action of the same step ahead of the drift (equal to the second while the opponent is 'greedy')."""
        N, Nc, Nt = self.num_envs, self.num_cameras, self.num_targets
        cam = torch.zeros((N, Nc, 2), dtype=torch.float64, device=self.device)
        tgt = torch.zeros((N, Nt, 2), dtype=torch.float64, device=self.device)
        check(self.lib.mate_engine_policy_actions(self._h, ctypes.c_void_p(cam.data_ptr()) if Nc else None,
                                                  ctypes.c_void_p(tgt.data_ptr()), self._stream()))
        if not greedy_targets:
            return cam, tgt
        greedy = torch.zeros((N, Nt, 2), dtype=torch.float64, device=self.device)
        check(self.lib.mate_engine_policy_greedy_target_actions(self._h, ctypes.c_void_p(greedy.data_ptr()), self._stream()))
        return cam, tgt, greedy

    def observe(self, tape_ct=None):
        io, keep = self._io(tape_ct=tape_ct)
        check(self.lib.mate_engine_observe(self._h, ctypes.byref(io), self._stream()))
        return self.camera_obs, self.target_obs

    def export_state(self, out=None):
        if out is None:
            out = torch.empty((self.num_envs, self.layout.export_width), dtype=torch.float64, device=self.device)
        check(self.lib.mate_engine_export_state(self._h, ctypes.c_void_p(out.data_ptr()), self._stream()))
        return out

    # ------------------------------------------------------------------ global state rows (centralised critics)
    def _state_affine(self, normalize):
        """Host (scale, bias) of mate.normalize_observation over the state space, as ctypes pointers (+ the arrays, to keep alive)."""
        if not normalize:
            return None, None, ()
        scale, bias = spaces.rescale_affine(consts.state_space_of(self.num_cameras, self.num_targets, self.num_obstacles))
        assert scale.shape == (self.state_dim,)
        return scale.ctypes.data_as(ctypes.c_void_p), bias.ctypes.data_as(ctypes.c_void_p), (scale, bias)

    def enable_state_rows(self, normalize=False, dtype=None):
        """Keep `Engine.state` ([N, state_dim], `dtype` = float32 / float64, default obs_dtype) current: the global state of every
        environment (MultiAgentTracking.state(), environment.py:894-906 of the reference), rewritten on the device as the last launch
        of every reset / step / observe / import_state / fused rollout (there: the state after the launch's last frame), raw or --
        `normalize` -- as mate.normalize_observation(state, state_space).  Call after the first reset().  Captured by the graphs a
        Stepper builds afterwards (a replay refreshes the tensor).  Returns the tensor, already filled."""
        dtype = dtype or self.obs_dtype
        assert dtype in (torch.float32, torch.float64)
        scale, bias, keep = self._state_affine(normalize)
        with torch.cuda.device(self.device):
            state = torch.zeros((self.num_envs, self.state_dim), dtype=dtype, device=self.device)
        check(self.lib.mate_engine_enable_state_rows(self._h, ctypes.c_void_p(state.data_ptr()), int(dtype == torch.float64), scale, bias))
        self.state, self.state_normalized = state, bool(normalize)
        return self.state_rows(out=state, normalize=normalize)

    def disable_state_rows(self):
        """Detach the state rows: the calls go back to their launch sequence without them; `Engine.state` becomes None."""
        check(self.lib.mate_engine_enable_state_rows(self._h, None, 0, None, None))
        self._clear_state_rows()

    def state_rows(self, out=None, normalize=False, dtype=None):
        """The global state rows of the current records, written by one launch on the current stream into `out` ([N, state_dim],
        float32 / float64, contiguous; default: a new tensor of `dtype`, default obs_dtype).  Nothing is attached."""
        if out is None:
            with torch.cuda.device(self.device):
                out = torch.empty((self.num_envs, self.state_dim), dtype=dtype or self.obs_dtype, device=self.device)
        assert out.dtype in (torch.float32, torch.float64) and out.is_contiguous() and out.device == self.device \
            and out.shape == (self.num_envs, self.state_dim)
        scale, bias, keep = self._state_affine(normalize)
        check(self.lib.mate_engine_state_rows(self._h, ctypes.c_void_p(out.data_ptr()), int(out.dtype == torch.float64), scale, bias, self._stream()))
        return out

    # ------------------------------------------------------------------ shaped reward rows (AuxiliaryCameraRewards / AuxiliaryTargetRewards)
    def enable_reward_rows(self, camera=None, target=None, dtype=torch.float64, accumulate=False, terms=False):
        """Keep the shaped per-agent rewards of the reference's AuxiliaryCameraRewards / AuxiliaryTargetRewards wrappers current on
        the device: `camera` / `target` = (coefficients dict, reduction) per team (None: that team is absent), as the torch shapers
        take them.  From now on every step / step_random / step_greedy / step_versus_greedy / fused rollout enqueues one more launch
        behind the stepping launch and AHEAD of the restart of finished episodes, which writes `camera_reward_rows` [N, Nc] and
        `target_reward_rows` [N, Nt] (`dtype`: float64 / float32) -- the rows describe the step `scalars` describes, the terminal one
        included, under every auto_reset -- and, with `terms`, every term into `camera_reward_terms` [N, Nc, 7] /
        `target_reward_terms` [N, Nt, 10] (f64; the order of AUXILIARY_REWARD_KEYS / ACCEPTABLE_KEYS: the reference's
        info['auxiliary_reward_<key>']).  `accumulate`: rows += shaped (FrameSkip's sum over per-step launches; zero the rows with
        `.zero_()` when consumed).  `reward_coefficients` = {'camera': [7], 'target': [10]} f64 device tensors the launch reads every
        time: writing into them in place applies a training-progress schedule, between the replays of a captured graph too.

        Call after the first reset(); a Stepper built afterwards captures the launches.  The stepping calls then need their masks
        output (step_random(want_masks=True), rollouts with want_masks=True).  Constant coefficients only: the reference's callable
        coefficients of (agent_id, episode_id, episode_step, ...) differ per environment and are out of scope.  A fused K-frame
        rollout leaves the rows of its LAST frame (sparse_delivery against the previous reward launch): per-frame shaped rewards
        inside one launch are out of scope -- FrameSkip with shaped rewards is K per-step launches in a graph with accumulate=True.
        Returns (camera_reward_rows, target_reward_rows)."""
        assert camera is not None or target is not None, 'enable_reward_rows needs at least one team'
        assert dtype in (torch.float32, torch.float64)
        tables = {team: reward_coefficient_table(team, *spec) for team, spec in (('camera', camera), ('target', target)) if spec is not None}
        soft = any('soft_coverage_score' in spec[0] for spec in (camera, target) if spec is not None)
        if soft:
            assert self.num_cameras > 0, 'soft_coverage_score needs cameras (the reference takes a max over them)'
            self.need_outer_boundary()
        N, agents, widths = self.num_envs, {'camera': self.num_cameras, 'target': self.num_targets}, {'camera': 7, 'target': 10}
        cfg = MateRewardRows()
        cfg.out_dtype, cfg.accumulate, cfg.soft_coverage = int(dtype == torch.float64), int(bool(accumulate)), int(soft)
        rows, term_rows, coefficients = {}, {}, {}
        with torch.cuda.device(self.device):
            for team, (table, reduction) in tables.items():
                # (a team without agents keeps a non-null pointer: the engine refuses it by name instead of taking it for absent)
                # (an empty view reports a null data_ptr(): the pointer is the buffer's own)
                buffer = torch.zeros(max(N * agents[team], 1), dtype=dtype, device=self.device)
                rows[team] = buffer[:N * agents[team]].view(N, agents[team])
                coefficients[team] = torch.tensor(table, dtype=torch.float64, device=self.device)
                setattr(cfg, team + '_rows_dev', buffer.data_ptr())
                setattr(cfg, team + '_coefficients_dev', coefficients[team].data_ptr())
                setattr(cfg, team + '_reduction', reduction)
                if terms:
                    term_rows[team] = torch.zeros((N, agents[team], widths[team]), dtype=torch.float64, device=self.device)
                    setattr(cfg, team + '_terms_dev', term_rows[team].data_ptr() or None)
        torch.cuda.current_stream(self.device).synchronize()      # (the tables are on the device before the engine's first launch reads them)
        check(self.lib.mate_engine_enable_reward_rows(self._h, ctypes.byref(cfg)))
        self.camera_reward_rows, self.target_reward_rows = rows.get('camera'), rows.get('target')
        self.camera_reward_terms, self.target_reward_terms = term_rows.get('camera'), term_rows.get('target')
        self.reward_coefficients, self.reward_accumulate = coefficients, bool(accumulate)
        self._forget_calls()
        return self.camera_reward_rows, self.target_reward_rows

    def disable_reward_rows(self):
        """Detach the reward rows: the calls go back to their launch sequence without them; the tensors become None."""
        check(self.lib.mate_engine_enable_reward_rows(self._h, None))
        self._clear_reward_rows()

    # ------------------------------------------------------------------ FrameSkip fragments behind the fused K-frame launch
    FRAGMENT_REWARDS = ('camera_team_reward', 'target_team_reward', 'normalized_target_team_reward', 'normalized_camera_team_reward')
    FRAGMENT_INFO = ('coverage_rate', 'real_coverage_rate', 'mean_transport_rate', 'num_delivered_cargoes')

    def _fragment_config(self, team, shaping, relative_coordinates, rescaled_observation, dtype, out):
        """(MateFragmentRows, what must stay alive during the call, a mask term has a non-zero coefficient) for `out`: the dict of output tensors."""
        code = _team_code(team)
        assert dtype in (torch.float32, torch.float64)
        name = ('camera', 'target')[code]
        cfg, keep = MateFragmentRows(), []
        cfg.team, cfg.out_dtype = code, int(dtype == torch.float64)
        for key in ('obs', 'rewards', 'info', 'done', 'frames', 'shaped'):
            tensor = out.get(key)
            if tensor is not None:
                assert tensor.is_contiguous() and tensor.device == self.device
                setattr(cfg, key + '_dev', tensor.data_ptr())
        masks = False
        if shaping is not None:
            table, cfg.reduction = reward_coefficient_table(name, *shaping)
            coefficients = np.ascontiguousarray(table, dtype=np.float64)
            cfg.coefficients = coefficients.ctypes.data
            keep.append(coefficients)
            masks = coefficients[5 if code == 0 else 7] != 0.0
        columns = spaces.fragment_column_table(name, self.num_cameras, self.num_targets, self.num_obstacles, relative_coordinates, rescaled_observation)
        if columns is not None:
            columns = [np.ascontiguousarray(c) for c in columns]
            cfg.column_sub, cfg.column_flag, cfg.column_scale, cfg.column_bias = (c.ctypes.data for c in columns)
            keep.append(columns)
        return cfg, keep, bool(masks)

    def _fragment_outputs(self, team, shaped, dtype):
        code = _team_code(team)
        N, A, D = self.num_envs, (self.num_cameras, self.num_targets)[code], (self.camera_obs_dim, self.target_obs_dim)[code]
        with torch.cuda.device(self.device):
            return {
                'obs': torch.zeros((N, A, D), dtype=self.obs_dtype, device=self.device),
                'rewards': torch.zeros((N, 4), dtype=torch.float64, device=self.device), 'info': torch.zeros((N, 4), dtype=torch.float64, device=self.device),
                'done': torch.zeros(N, dtype=torch.uint8, device=self.device), 'frames': torch.zeros(N, dtype=torch.int32, device=self.device),
                'shaped': torch.zeros((N, A), dtype=dtype, device=self.device) if shaped else None,
            }

    def enable_fragment_rows(self, team, frame_skip, shaping=None, relative_coordinates=False, rescaled_observation=False, dtype=torch.float64,
                             first_rows=False, final_obs=False, per_frame=False):
        """Attach the tail of the example trainers' wrapper chain -- RelativeCoordinates -> RescaledObservation ->
        RepeatedRewardIndividualDone -> [AuxiliaryCameraRewards | AuxiliaryTargetRewards] -> FrameSkip(frame_skip) -- to the fused
        K-frame launch: from now on rollout_versus_greedy(team, ...) (and a Stepper(versus=team, frame_skip=K) built afterwards)
        enqueues ONE more launch behind the stepping launch and ahead of the restart, which reduces the launch's K frames to what
        FrameSkip hands the learner, in engine-owned tensors:
          fragment_obs [N, A, D] (obs_dtype): the rows of the last frame that ran, through RelativeCoordinates / RescaledObservation
            when asked for (the fused launch itself packs plain rows: do NOT call set_obs_transform), bit-identical to the per-step
            flows' transformed rows;
          fragment_rewards [N, 4] f64 (FRAGMENT_REWARDS), fragment_done [N] u8, fragment_frames [N] int32 (frames that ran),
          fragment_info [N, 4] f64 (FRAGMENT_INFO: means of the two coverage rates, the last frame's transport rate and deliveries),
          fragment_shaped [N, A] (`dtype`) with `shaping` = (coefficients dict, reduction): the sum over the frames of the shaped
            rows, equal to per-step launches with enable_reward_rows(accumulate=True); FRAGMENT_REFUSED_KEYS are refused,
          fragment_coefficients [7] / [10] f64: the engine's device table, rewritten in place by a schedule (between graph replays too).
        An environment that ran no frame (idle under a batched restart) keeps its fragment_obs row; its other rows are 0.  A fused launch
        restarts finished episodes behind the launch without packing their first observation: a restarted environment hands the
        learner its terminal row, done set, for one fragment (as FrameSkip does before the trainer's reset()), and the next action
        is chosen on that row -- unless `first_rows` is on (mate_engine_enable_first_rows).  Then, after every such call, for the
        environments it restarted (fragment_restarted [N] bool = fragment_first_scalars[:, 2] != 2): their fragment_obs row is the new
        episode's FIRST row through the same transform -- env.reset()'s row of the reference's trainers, what the per-step flows hand
        over in the restarting call, bit for bit -- also where the environment ran no frame in this fragment; with `final_obs`,
        fragment_final_obs [N, A, D] holds for them what fragment_obs would have shown without the feature (the terminal row, or the row
        kept while idling under a batched interval).  done, frames, rewards, info and shaped are unchanged, and so is every row of an
        environment that was not restarted (its fragment_final_obs row is untouched).  fragment_first_rows [N, A, D] is the working
        buffer of the plain first rows, fragment_first_scalars [N, 8] f32 the restart's own records (2.0 where nothing restarted).
        Costs one memset node and one or two K = 1 launches of the fragment kernel per call; no stepping kernel changes.  A restart that
        closes an interval because auto_reset or the flow changed (at the head of a later call) delivers no first rows.
        `per_frame` = True builds the SAME tensors frame by frame instead (mate_engine_enable_frame_fragments): one small launch behind each
        step_versus_greedy(team, ...) call folds that frame in, a fragment is `frame_skip` such calls (step_fragment_frames, or a
        Stepper(versus=team, frame_skip=K) built afterwards) under auto_reset = a multiple of K -- against ANY opponent the per-step flows
        have (Heuristic, mixtures, channels).  `shaping` then attaches the team's reward rows in overwrite mode (enable_reward_rows) and
        allows all of its terms (soft_coverage_score still needs the outer boundary); fragment_coefficients is that launch's table.
        relative_coordinates / rescaled_observation set the packer's transform (set_obs_transform): the rows arrive transformed, there is
        no column table.  With `first_rows` the dict gains 'restarted' [N] u8 and (`final_obs`) 'final_obs'; there are no first-row working
        buffers, since the per-step restart packs the first rows into the call's own.  Against the Greedy opponents every tensor equals
        the fused fragment's bit for bit.
        Call after the first reset().  Returns fragment_obs."""
        frame_skip = int(frame_skip)
        assert frame_skip >= 1
        assert first_rows or not final_obs, 'final_obs belongs to first_rows = True'
        if per_frame:
            return self._enable_frame_fragments(team, frame_skip, shaping, relative_coordinates, rescaled_observation, dtype, first_rows, final_obs)
        out = self._fragment_outputs(team, shaping is not None, dtype)
        cfg, keep, masks = self._fragment_config(team, shaping, relative_coordinates, rescaled_observation, dtype, out)
        torch.cuda.current_stream(self.device).synchronize()
        check(self.lib.mate_engine_enable_fragment_rows(self._h, ctypes.byref(cfg)))
        ptr, count = ctypes.c_void_p(), ctypes.c_int32()
        check(self.lib.mate_engine_fragment_coefficients(self._h, ctypes.byref(ptr), ctypes.byref(count)))
        self._fragment_coefficients_view = (ptr.value, count.value, '<f8', (count.value,)) if shaping is not None else None
        self.fragment_obs, self.fragment_rewards, self.fragment_done = out['obs'], out['rewards'], out['done']
        self.fragment_frames, self.fragment_info, self.fragment_shaped = out['frames'], out['info'], out['shaped']
        self.fragment_team, self.fragment_frame_skip, self._fragment_masks = cfg.team, frame_skip, masks
        self._clear_first_rows()
        check(self.lib.mate_engine_enable_first_rows(self._h, None))
        if first_rows:
            with torch.cuda.device(self.device):
                rows, scalars = torch.zeros_like(out['obs']), torch.full((self.num_envs, 8), 2.0, dtype=torch.float32, device=self.device)
                final = torch.zeros_like(out['obs']) if final_obs else None
            first = MateFirstRows(rows.data_ptr(), scalars.data_ptr(), final.data_ptr() if final_obs else None)
            torch.cuda.current_stream(self.device).synchronize()
            check(self.lib.mate_engine_enable_first_rows(self._h, ctypes.byref(first)))
            self.fragment_first_rows, self.fragment_first_scalars, self.fragment_final_obs = rows, scalars, final
        self.reserve_rollout(frame_skip, want_masks=masks)
        return self.fragment_obs

    def _enable_frame_fragments(self, team, frame_skip, shaping, relative_coordinates, rescaled_observation, dtype, first_rows, final_obs):
        code = _team_code(team)
        name = ('camera', 'target')[code]
        assert dtype in (torch.float32, torch.float64)
        if self.fragment_team is not None:
            self.disable_fragment_rows()
        self.set_obs_transform(relative_coordinates=relative_coordinates, rescaled_observation=rescaled_observation)
        if shaping is not None:
            self.enable_reward_rows(**{name: shaping}, dtype=dtype, accumulate=False)
        out = self._fragment_outputs(code, shaping is not None, dtype)
        with torch.cuda.device(self.device):
            restarted = torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device) if first_rows else None
            final = torch.zeros_like(out['obs']) if final_obs else None
        cfg = MateFrameFragments()
        cfg.team, cfg.frames, cfg.out_dtype, cfg.first_rows = code, frame_skip, int(dtype == torch.float64), int(bool(first_rows))
        for key, tensor in dict(out, final_obs=final, restarted=restarted).items():
            if tensor is not None:
                setattr(cfg, key + '_dev', tensor.data_ptr())
        torch.cuda.current_stream(self.device).synchronize()
        check(self.lib.mate_engine_enable_frame_fragments(self._h, ctypes.byref(cfg)))
        self.fragment_obs, self.fragment_rewards, self.fragment_done = out['obs'], out['rewards'], out['done']
        self.fragment_frames, self.fragment_info, self.fragment_shaped = out['frames'], out['info'], out['shaped']
        self.fragment_team, self.fragment_frame_skip, self._fragment_masks = code, frame_skip, False
        self.fragment_per_frame, self._frame_restarted, self.fragment_final_obs = True, restarted, final
        self._forget_calls()
        return self.fragment_obs

    def frame_fragment(self, team, rows, scalars, phase, frame_skip, closes=False, out=None, dtype=torch.float64):
        """The frame launch on demand over caller buffers (mate_engine_frame_fragment): `rows` [N, A, D] (obs_dtype) the team's rows of ONE frame,
        `scalars` [N, 8] f32 its records, folded as frame `phase` of `frame_skip` into `out` -- a dict of tensors by the fragment's names (any subset
        of obs, rewards, info, done, frames, shaped, final_obs, restarted; None: new ones, without shaped) that the NEXT phases keep adding to.
        `closes`: the second form instead -- `rows` are the first rows of what the record says finished.  'shaped' sums the attached reward rows.
        Returns `out`."""
        code = _team_code(team)
        if out is None:
            out = {k: v for k, v in self._fragment_outputs(code, False, dtype).items() if v is not None}
        cfg = MateFrameFragments()
        cfg.team, cfg.frames, cfg.out_dtype = code, int(frame_skip), int(dtype == torch.float64)
        for key, tensor in out.items():
            assert tensor.is_contiguous() and tensor.device == self.device
            setattr(cfg, key + '_dev', tensor.data_ptr())
        assert rows.is_contiguous() and rows.dtype == self.obs_dtype and scalars.is_contiguous() and scalars.dtype == torch.float32
        io = MateStepIO()
        io.scalars_dev = scalars.data_ptr()
        setattr(io, ('camera', 'target')[code] + '_obs_dev', rows.data_ptr())
        check(self.lib.mate_engine_frame_fragment(self._h, ctypes.byref(cfg), ctypes.byref(io), int(phase), int(bool(closes)), self._stream()))
        return out

    def step_fragment_frames(self, team, joint_action, auto_reset=None, policy_tape=None):
        """One learner step of FrameSkip(K) over the per-frame fragments (enable_fragment_rows(per_frame=True)): K calls of
        step_versus_greedy(team, joint_action) with the action held, under `auto_reset` (a multiple of K; default K: finished environments
        idle to their fragment's end and restart behind it).  Returns the fragment dict."""
        code = _team_code(team)
        assert self.fragment_per_frame and self.fragment_team == code, 'enable_fragment_rows(team, K, per_frame=True) first'
        K = self.fragment_frame_skip
        auto_reset = K if auto_reset is None else int(auto_reset)
        for _ in range(K):
            self.step_versus_greedy(code, joint_action, policy_tape=policy_tape, auto_reset=auto_reset)
        return self.fragment

    def disable_fragment_rows(self):
        """Detach the fragment launch (and the first rows with it): rollout_versus_greedy goes back to its launch sequence without it; the tensors become None.
        The per-frame form: step_versus_greedy goes back to its own (reward rows it attached for `shaping` stay: disable_reward_rows)."""
        check(self.lib.mate_engine_enable_fragment_rows(self._h, None))
        check(self.lib.mate_engine_enable_frame_fragments(self._h, None))
        self._clear_fragment_rows()

    # ------------------------------------------------------------------ per-episode metric records
    EPISODE_COLUMNS = ('env', 'episode', 'steps', 'frames', 'length', 'episode_raw_reward', 'episode_normalized_raw_reward', 'episode_reward',
                       'raw_reward', 'normalized_raw_reward', 'coverage_rate', 'real_coverage_rate', 'mean_transport_rate', 'num_delivered_cargoes',
                       'num_tracked', 'team')

    def enable_episode_records(self, team, capacity=None):
        """Attach the episode launch (mate_engine_enable_episode_records): behind every stepping call the engine adds the call's learner
        steps -- its frames; a fragment counts as its frames -- to per-environment
        running sums and appends one record of EPISODE_COLUMNS (the reference's CustomMetricCallback keys, for `team`'s perspective) to
        episode_ring [capacity, 16] f64 whenever an episode ends; episode_count [1] int64 counts the records ever appended, record n lives
        in row n % capacity.  capacity defaults to max(4 num_envs, 1024); below num_envs the launch serialises.  num_tracked is kept for
        the camera team where the calls bring masks (want_masks), NaN otherwise.  Call after the first reset().  Returns episode_ring."""
        code = _team_code(team)
        capacity = max(4 * self.num_envs, 1024) if capacity is None else int(capacity)
        with torch.cuda.device(self.device):
            ring = torch.zeros((max(capacity, 1), len(self.EPISODE_COLUMNS)), dtype=torch.float64, device=self.device)
            count = torch.zeros(1, dtype=torch.int64, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()
        check(self.lib.mate_engine_enable_episode_records(self._h, code, ctypes.c_void_p(ring.data_ptr()), capacity, ctypes.c_void_p(count.data_ptr())))
        self.episode_ring, self.episode_count, self.episode_team, self._episode_read = ring, count, code, 0
        return self.episode_ring

    def disable_episode_records(self):
        """Detach the episode launch: every flow goes back to its launch sequence without it; the tensors become None."""
        check(self.lib.mate_engine_enable_episode_records(self._h, 0, None, 0, None))
        self._clear_episode_records()

    def clear_episode_records(self):
        """Forget the episodes in progress (their next records start from this call); the ring and the count stay."""
        check(self.lib.mate_engine_clear_episode_records(self._h, self._stream()))

    def episode_records(self):
        """(records, dropped): the records appended since the last call, oldest first, [M, 16] f64 on the device (a copy), and how many
        more were overwritten in the ring before they were read.  Waits for the stream's launches."""
        assert self.episode_ring is not None, 'call enable_episode_records() first'
        torch.cuda.current_stream(self.device).synchronize()
        total, capacity = int(self.episode_count.item()), self.episode_ring.shape[0]
        fresh = total - self._episode_read
        kept = min(fresh, capacity)
        rows = torch.arange(total - kept, total, dtype=torch.int64, device=self.device) % capacity
        self._episode_read = total
        return self.episode_ring[rows], fresh - kept

    # ------------------------------------------------------------------ MoreTrainingInformation rows
    INFO_CAMERA_COLUMNS = ('num_tracked', 'is_sensed')
    INFO_TARGET_COLUMNS = ('goal', 'goal_distance') + tuple(f'warehouse_distances_{w}' for w in range(4)) + ('individual_done', 'is_tracked', 'is_colliding')
    INFO_CARGO_COLUMNS = (tuple(f'remaining_cargo_counts_{w}' for w in range(4)) + tuple(f'awaiting_cargo_counts_{w}' for w in range(4)) +
                          tuple(f'remaining_cargoes_{w}_{d}' for w in range(4) for d in range(4)))

    def _info_tensors(self, camera, target, cargo):
        """Fresh (camera, target, cargo) row tensors, None for an output that is off (`camera` is off without cameras)."""
        N, Nc, Nt = self.num_envs, self.num_cameras, self.num_targets
        with torch.cuda.device(self.device):
            new = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=self.device)  # noqa: E731
            return (new(N, Nc, len(self.INFO_CAMERA_COLUMNS)) if camera and Nc else None,
                    new(N, Nt, len(self.INFO_TARGET_COLUMNS)) if target else None,
                    new(N, len(self.INFO_CARGO_COLUMNS)) if cargo else None)

    @staticmethod
    def _row_pointers(rows):
        return [ctypes.c_void_p(r.data_ptr()) if r is not None else None for r in rows]

    def enable_info_rows(self, camera=True, target=True, cargo=True):
        """Keep what the reference's mate.MoreTrainingInformation wrapper adds to the agents' infos current on the device
        (mate_engine_enable_info_rows): from now on every stepping call enqueues one more launch behind the stepping launch and AHEAD
        of the restart of finished episodes, which writes `info_camera_rows` [N, Nc, 2] (INFO_CAMERA_COLUMNS), `info_target_rows`
        [N, Nt, 9] (INFO_TARGET_COLUMNS) and `info_cargo_rows` [N, 24] (INFO_CARGO_COLUMNS), all f64 -- the rows describe the step
        `scalars` describes, the terminal one included; info() names the columns.  The tensors are allocated once and are the same at
        every call; `camera` is silently off without cameras.  A fused K-frame rollout leaves the rows of its LAST frame with
        individual_done = NaN.  Call after the first reset(); a Stepper built afterwards captures the launch.  The stepping calls then
        need their masks output (step_random(want_masks=True), rollouts with want_masks=True).  Returns the three tensors."""
        wanted = (bool(camera) and self.num_cameras > 0, bool(target), bool(cargo))
        assert any(wanted), 'enable_info_rows needs at least one output'
        have = (self.info_camera_rows, self.info_target_rows, self.info_cargo_rows)
        fresh = self._info_tensors(*[w and h is None for w, h in zip(wanted, have)])
        rows = tuple((h if h is not None else f) if w else None for w, h, f in zip(wanted, have, fresh))
        torch.cuda.current_stream(self.device).synchronize()
        check(self.lib.mate_engine_enable_info_rows(self._h, *self._row_pointers(rows)))
        self.info_camera_rows, self.info_target_rows, self.info_cargo_rows = rows
        self._forget_calls()
        return rows

    def _info_attached(self):
        return self.info_camera_rows is not None or self.info_target_rows is not None or self.info_cargo_rows is not None

    def disable_info_rows(self):
        """Detach the training-information rows: the calls go back to their launch sequence without them; the tensors become None."""
        check(self.lib.mate_engine_enable_info_rows(self._h, None, None, None))
        self._clear_info_rows()

    def info_rows(self, masks=None):
        """(camera [N, Nc, 2] or None without cameras, target [N, Nt, 9], cargo [N, 24]): the rows of the CURRENT records by one launch on
        the current stream, in fresh tensors; nothing is attached.  individual_done reads NaN (no previous step to compare with);
        `masks` = the packed mask words [N, mask_words] of those records (Engine.masks behind a step that brought them), None: num_tracked,
        is_sensed and is_tracked read NaN."""
        if masks is not None:
            assert masks.dtype == torch.int32 and masks.is_contiguous() and masks.device == self.device and masks.shape == (self.num_envs, self.layout.mask_words)
        rows = self._info_tensors(True, True, True)
        check(self.lib.mate_engine_info_rows(self._h, ctypes.c_void_p(masks.data_ptr()) if masks is not None else None, *self._row_pointers(rows), self._stream()))
        return rows

    # ------------------------------------------------------------------ off-screen render (MultiAgentTracking.render(mode='rgb_array'))
    RENDER_SIZES = (16, 4096)      # MATE_RENDER_MIN_SIZE, MATE_RENDER_MAX_SIZE

    def keep_masks(self):
        """Have the engine keep its own copy of the packed mask words (mate_engine_keep_masks): every later launch that writes a view fills it, whether the
        call brings its masks output or not.  What render() reads; call it ahead of the reset.  enable_policies() allocates the same copy."""
        check(self.lib.mate_engine_keep_masks(self._h))
        self._own_masks = True

    def render(self, envs=None, size=800, headings=None, out=None):
        """uint8 [k, size, size, 3] on the device: the reference's render(mode='rgb_array') pictures of the environments `envs` (indices into this
        engine's batch, any order, repeats allowed; None: all of them) by ONE launch on the current stream, from the CURRENT records and the engine's
        own mask words (what is drawn, what is not).  `headings`: [k, Nt] degrees, the reference's render-only
        target_orientations of each requested frame (None: zeros).  `out`: a contiguous uint8 [k, size, size, 3] tensor to write instead of a new one.
        It reads, and writes nothing but the frames.  The engine keeps its own mask words from keep_masks() (or enable_policies()) on: call it ahead of
        the reset, as both environment classes do; without it the call is refused (EngineError, MATE_ESTATE).  With `envs` given the indices are uploaded at
        every call, so only `envs=None` into a preallocated `out` is capturable."""
        lo, hi = self.RENDER_SIZES
        size = int(size)
        if not lo <= size <= hi:
            raise ValueError(f'render: size must lie in [{lo}, {hi}], got {size}')
        if envs is None:
            index, k = None, self.num_envs
        else:
            host = np.asarray(envs.cpu() if torch.is_tensor(envs) else envs, dtype=np.int64).reshape(-1)
            if host.size < 1 or host.min() < 0 or host.max() >= self.num_envs:
                raise ValueError(f'render: the environments must be indices in [0, {self.num_envs}) and at least one, got {host.tolist()}')
            index, k = torch.from_numpy(host.astype(np.int32)).to(self.device), int(host.size)
        if headings is not None:
            headings = torch.as_tensor(headings, dtype=torch.float64).to(self.device).contiguous()
            if headings.shape != (k, self.num_targets):
                raise ValueError(f'render: headings must be [{k}, {self.num_targets}], got {tuple(headings.shape)}')
        if out is None:
            with torch.cuda.device(self.device):
                out = torch.empty((k, size, size, 3), dtype=torch.uint8, device=self.device)
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.device == self.device and out.shape == (k, size, size, 3)
        check(self.lib.mate_engine_render(self._h, ctypes.c_void_p(index.data_ptr()) if index is not None else None, k, size,
                                          ctypes.c_void_p(headings.data_ptr()) if headings is not None else None, ctypes.c_void_p(out.data_ptr()), self._stream()))
        return out

    # ------------------------------------------------------------------ communication arrows (mate/wrappers/render_communication.py: RenderCommunication)
    def enable_communication_trace(self, teams=('camera', 'target'), duration=20, channels=True):
        """Keep RenderCommunication's state on the device (mate_engine_enable_comm_trace): per team of `teams` a uint8 matrix
        remaining[N, sender, recipient], counted down at every live per-step call and set to `duration` (1 .. 255) wherever a message was delivered since the
        previous step; render() then draws the wrapper's dashed arrows, cameras blue and targets red, behind the obstacles and under the sectors.  The
        learner's own messages (enable_messages / route_messages) are seen as they are.  A team the ENGINE plays materialises its agents' edges only where
        its agents' launch runs under a channel, so with the on-device agents enabled this call installs a transparent channel -- set_channel(team), every
        message arrives -- for every team of `teams` that has none (step_greedy / step_versus_greedy then take the two-launch form); where set_channel
        refuses the team (a seat, the Heuristic camera agent) so does this call.  While enabled the fused rollouts (rollout_random, rollout_greedy,
        rollout_versus_greedy, frame_skip > 1 steppers) and pipelined restarts are refused: step per frame.  The matrices start from zeros; every reset and
        restart starts its environments from zeros again.  channels=False: install no channel (the caller plants the matrices itself).  teams=(): detach."""
        codes = sorted({_team_code(t) for t in teams})
        duration = int(duration)
        if codes and not 1 <= duration <= 255:
            raise ValueError(f'enable_communication_trace: duration must lie in [1, 255], got {duration}')
        for team in codes:
            if (self.num_cameras, self.num_targets)[team] == 0:
                raise ValueError(f"enable_communication_trace: the scenario has no {('camera', 'target')[team]}s to talk")
        installed = []
        try:
            if self._policies and channels:
                for team in codes:
                    if self.channels[team] is None:
                        self.set_channel(team)
                        installed.append(team)
            check(self.lib.mate_engine_enable_comm_trace(self._h, sum(1 << t for t in codes), duration if codes else 0))
        except Exception:      # (a refused call changes nothing: the channels it installed go again)
            for team in installed:
                self.clear_channel(team)
            raise
        self.trace_duration, self.trace_teams = (duration, tuple(codes)) if codes else (0, ())

    def disable_communication_trace(self):
        """Detach the trace (a channel enable_communication_trace installed stays: clear_channel removes it)."""
        self.enable_communication_trace(teams=())

    def communication_trace(self, team):
        """The team's remaining[N, n, n] as a zero-copy uint8 view of the engine-owned matrix, [sender][recipient] (mate_engine_comm_trace).  An environment
        whose episode has changed since its last live step still shows the old episode's bytes until its next step; communication_trace_tags() says which."""
        return self._trace_views(team)[0]

    def communication_trace_tags(self, team):
        """int32 [N]: the episode number each environment's matrix belongs to (-1: none yet); render() draws a matrix only where it is the current one."""
        return self._trace_views(team)[1]

    def _trace_views(self, team):
        team = _team_code(team)
        n, N = (self.num_cameras, self.num_targets)[team], self.num_envs
        remaining, tags = ctypes.c_void_p(), ctypes.c_void_p()
        check(self.lib.mate_engine_comm_trace(self._h, team, ctypes.byref(remaining), ctypes.byref(tags)))
        return (torch.as_tensor(_EngineOwned(self, remaining.value, N * n * n, '|u1'), device=self.device).view(N, n, n),
                torch.as_tensor(_EngineOwned(self, tags.value, N, '<i4'), device=self.device))

    def set_communication_trace(self, team, remaining):
        """Plant `remaining` ([N, n, n] uint8, [sender][recipient]; host or device) as the team's matrix, tagged with the environments' current episodes
        (mate_engine_set_comm_trace): what the next render() draws.  The N = 1 class's host mailbox and the tests come here."""
        team = _team_code(team)
        n = (self.num_cameras, self.num_targets)[team]
        value = torch.from_numpy(np.array(remaining.cpu().numpy() if torch.is_tensor(remaining) else remaining, dtype=np.uint8, order='C')).to(self.device)
        self._check_tensor('remaining', value, torch.uint8, (self.num_envs, n, n))
        torch.cuda.current_stream(self.device).synchronize()      # (the upload is complete before the engine's own stream copies it)
        check(self.lib.mate_engine_set_comm_trace(self._h, team, ctypes.c_void_p(value.data_ptr())))

    @staticmethod
    def info_views(camera_rows, target_rows, cargo_rows):
        """{name: view} over the three row tensors (None: that output's names are absent): [N, Nc] / [N, Nt] columns,
        warehouse_distances [N, Nt, 4], remaining_cargo_counts / awaiting_cargo_counts [N, 4], remaining_cargoes [N, 4, 4]."""
        out = {}
        if camera_rows is not None:
            out.update(num_tracked=camera_rows[:, :, 0], is_sensed=camera_rows[:, :, 1])
        if target_rows is not None:
            out.update(goal=target_rows[:, :, 0], goal_distance=target_rows[:, :, 1], warehouse_distances=target_rows[:, :, 2:6],
                       individual_done=target_rows[:, :, 6], is_tracked=target_rows[:, :, 7], is_colliding=target_rows[:, :, 8])
        if cargo_rows is not None:
            out.update(remaining_cargo_counts=cargo_rows[:, 0:4], awaiting_cargo_counts=cargo_rows[:, 4:8],
                       remaining_cargoes=cargo_rows[:, 8:24].view(-1, 4, 4))
        return out

    def info(self):
        """{name: view} over the attached rows (enable_info_rows), see info_views; the same storage at every call."""
        assert self._info_attached(), 'call enable_info_rows() first'
        return self.info_views(self.info_camera_rows, self.info_target_rows, self.info_cargo_rows)

    @property
    def fragment_restarted(self):
        """[N] bool: the environments the last rollout_versus_greedy of the attached team restarted -- whose fragment_obs row is the new
        episode's first row (enable_fragment_rows(first_rows=True)); None while first rows are off.  A new tensor at every read."""
        if self.fragment_per_frame:
            return None if self._frame_restarted is None else self._frame_restarted != 0
        if self.fragment_first_scalars is None:
            return None
        return self.fragment_first_scalars[:, 2] != 2

    @property
    def fragment(self):
        """The fragment tensors by name (None while detached)."""
        if self.fragment_team is None:
            return None
        out = {'obs': self.fragment_obs, 'rewards': self.fragment_rewards, 'done': self.fragment_done, 'frames': self.fragment_frames,
               'info': self.fragment_info, 'shaped': self.fragment_shaped, 'coefficients': self.fragment_coefficients}
        if self.fragment_per_frame:
            if self.fragment_shaped is not None:
                out['coefficients'] = self.reward_coefficients[('camera', 'target')[self.fragment_team]]
            if self._frame_restarted is not None:
                out.update(restarted=self._frame_restarted, final_obs=self.fragment_final_obs)
        if self.fragment_first_scalars is not None:      # (first rows on: the keys exist only then)
            out.update(first_rows=self.fragment_first_rows, first_scalars=self.fragment_first_scalars, final_obs=self.fragment_final_obs)
        return out

    def fragment_rows(self, team, rows, scalars, masks=None, shaping=None, relative_coordinates=False, rescaled_observation=False,
                      dtype=torch.float64, out=None):
        """The fragment launch on demand over caller buffers: `rows` [K, N, A, D] (obs_dtype) the team's PLAIN observation rows,
        `scalars` [K, N, 8] f32, `masks` [K, N, mask_words] int32 (needed by num_tracked / is_tracked).  K = 1 over the engine's
        per-step tensors gives the transformed reset() observation.  `out`: a dict of tensors to write (as returned); default: new
        ones.  Returns {'obs', 'rewards', 'info', 'done', 'frames', 'shaped'}."""
        code = _team_code(team)
        if rows.dim() == 3:
            rows, scalars, masks = rows[None], scalars[None], (masks[None] if masks is not None else None)
        K = int(rows.shape[0])
        N, A, D = self.num_envs, (self.num_cameras, self.num_targets)[code], (self.camera_obs_dim, self.target_obs_dim)[code]
        assert rows.shape == (K, N, A, D) and rows.dtype == self.obs_dtype and rows.is_contiguous() and rows.device == self.device
        assert scalars.shape == (K, N, 8) and scalars.dtype == torch.float32 and scalars.is_contiguous() and scalars.device == self.device
        if out is None:
            out = self._fragment_outputs(code, shaping is not None, dtype)
        cfg, keep, _ = self._fragment_config(code, shaping, relative_coordinates, rescaled_observation, dtype, out)
        if masks is not None:
            assert masks.shape == (K, N, self.layout.mask_words) and masks.dtype == torch.int32 and masks.is_contiguous() and masks.device == self.device
        io = self._bind_outputs(MateStepIO(), rows if code == 0 else None, rows if code == 1 else None, scalars, masks)
        torch.cuda.current_stream(self.device).synchronize()
        check(self.lib.mate_engine_fragment_rows(self._h, ctypes.byref(cfg), ctypes.byref(io), K, self._stream()))
        return out

    # ------------------------------------------------------------------ target-selection camera actions (HierarchicalCamera)
    SELECTION_METRICS = ('num_selected_targets', 'num_valid_selected_targets', 'num_invalid_selected_targets', 'invalid_target_selection_rate')

    def encode_selection(self, selection, multi_selection=None):
        """encode_selection() of this module for this engine's shape, on its device."""
        multi = self.multi_selection if multi_selection is None else bool(multi_selection)
        return encode_selection(selection, multi, self.num_envs, self.num_cameras, self.num_targets, device=self.device)

    def enable_selection(self, multi_selection=True, selection=None, accumulate=False, act_dtype=torch.float64):
        """Attach the executor of the reference's HierarchicalCamera wrapper (examples/hrl/wrappers.py): from now on step_selected()
        turns `Engine.selection` ([N, Nc] int32: bit t = target t selected, or -- single selection -- an index in [0, Nt], Nt = none)
        into the camera team's joint action on the device (`selection_actions` [N, Nc, 2]), steps against the greedy targets, and
        leaves the wrapper's four metrics in `selection_metrics` [N, Nc, 4] f64 (SELECTION_METRICS), the frames that contributed in
        `selection_frames` [N] int32 and action_mask() of the next observation in `action_mask` ([N, Nc, 2 Nt] / [N, Nc, Nt + 1] u8).
        `accumulate`: metrics and frames add up over calls (FrameSkip: mean = metrics / frames; zero both when consumed).  `selection`: a
        caller-owned int32 [N, Nc] tensor to read instead of a new one.  Needs enable_policies() and a reset() since.  Returns the
        selection tensor."""
        N, Nc, Nt = self.num_envs, self.num_cameras, self.num_targets
        assert act_dtype in (torch.float32, torch.float64)
        with torch.cuda.device(self.device):
            if selection is None:
                selection = torch.full((N, Nc), 0 if multi_selection else Nt, dtype=torch.int32, device=self.device)
            assert selection.dtype == torch.int32 and selection.shape == (N, Nc) and selection.is_contiguous() and selection.device == self.device, \
                'selection: a contiguous int32 [num_envs, num_cameras] tensor on the engine device'
            metrics = torch.zeros((N, Nc, 4), dtype=torch.float64, device=self.device)
            frames = torch.zeros(N, dtype=torch.int32, device=self.device)
            action_mask = torch.zeros((N, Nc, 2 * Nt if multi_selection else Nt + 1), dtype=torch.uint8, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()
        flags = (1 if accumulate else 0) | (2 if act_dtype == torch.float32 else 0)
        check(self.lib.mate_engine_enable_selection(self._h, int(bool(multi_selection)), ctypes.c_void_p(selection.data_ptr()), ctypes.c_void_p(metrics.data_ptr()),
                                                    ctypes.c_void_p(frames.data_ptr()), ctypes.c_void_p(action_mask.data_ptr()), flags))
        ptr, code = ctypes.c_void_p(), ctypes.c_int32()
        check(self.lib.mate_engine_selection_actions(self._h, ctypes.byref(ptr), ctypes.byref(code)))
        # the engine-owned joint action as a zero-copy tensor (the engine outlives it: the tensor keeps `self`; built at every read)
        self._selection_actions_view = (ptr.value, N * Nc * 2, '<f8' if code.value == 1 else '<f4', (N, Nc, 2))
        self.selection, self.selection_metrics, self.selection_frames, self.action_mask = selection, metrics, frames, action_mask
        self.multi_selection, self.selection_accumulate = bool(multi_selection), bool(accumulate)
        return selection

    def disable_selection(self):
        check(self.lib.mate_engine_disable_selection(self._h))
        self._clear_selection()

    def step_selected(self, policy_tape=None, tape_ct=None, tape_goal=None, auto_reset=True):
        """One frame of HierarchicalCamera over MultiCamera(target_agent=GreedyTargetAgent()): the executor turns `Engine.selection` into
        the cameras' joint action, the greedy targets act, the environment steps; metrics, action mask and the attached rows follow
        (mate_engine_step_selected).  Returns (camera_obs, target_obs, scalars)."""
        io, keep = self._io(tape_ct=tape_ct, tape_goal=tape_goal)
        check(self.lib.mate_engine_step_selected(self._h, ctypes.byref(io), self._policy_tape(policy_tape, keep), int(auto_reset), self._stream()))
        return self.camera_obs, self.target_obs, self.scalars

    # One copy per step for the N = 1 NumPy API (mate_amd.environment): the output tensors and an export_state buffer become views of
    # ONE device allocation, and fetch_host() brings a step's results over in a single transfer (five blocking copies of a few KB each
    # were a third of that API's 250 us per step).
    def stage_outputs(self):
        """Re-home camera_obs / target_obs / scalars / masks (and a state-export buffer) in one flat device buffer.  Call before
        the first reset; the tensors keep their names, shapes and dtypes."""
        parts = [('camera_obs', self.camera_obs), ('target_obs', self.target_obs), ('scalars', self.scalars), ('masks', self.masks),
                 ('state', torch.empty((self.num_envs, self.layout.export_width), dtype=torch.float64, device=self.device))]
        offsets, total = [], 0
        for _, t in parts:
            offsets.append(total)
            total += -(-t.numel() * t.element_size() // 256) * 256
        flat = torch.zeros(total, dtype=torch.uint8, device=self.device)
        self._staged = {'flat': flat, 'views': {}}
        for (name, t), off in zip(parts, offsets):
            nbytes = t.numel() * t.element_size()
            view = flat[off:off + nbytes].view(t.dtype).view(t.shape)
            self._staged['views'][name] = (off, nbytes, t.dtype, tuple(t.shape))
            if name == 'state':
                self._staged['state'] = view
            else:
                setattr(self, name, view)
        self._forget_calls()

    _NP = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32}

    def fetch_host(self):
        """(after stage_outputs) the current state exported + ONE device-to-host copy: dict of NumPy arrays camera_obs, target_obs,
        scalars, masks, state -- views of one host buffer, valid until the next call."""
        self.export_state(out=self._staged['state'])
        pinned = self._staged.get('pinned')
        if pinned is None:
            pinned = self._staged['pinned'] = torch.empty(self._staged['flat'].shape, dtype=torch.uint8, pin_memory=True)
        pinned.copy_(self._staged['flat'], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        host = pinned.numpy().copy()          # (the caller keeps views of it; the pinned buffer is rewritten by the next call)
        return {name: host[off:off + nbytes].view(self._NP[dtype]).reshape(shape)
                for name, (off, nbytes, dtype, shape) in self._staged['views'].items()}

    def state_dict_from(self, flat):
        """state_dict() of an already fetched [N, export_width] f64 array."""
        if self._export_slices is None:
            self._export_slices = [(name, off, int(np.prod(shape)) if shape else 1, (self.num_envs,) + tuple(shape))
                                   for name, (off, shape) in self.export_fields.items()]
        return {name: flat[:, off:off + n].reshape(shape) for name, off, n, shape in self._export_slices}

    def import_state(self, flat):
        flat = flat.to(device=self.device, dtype=torch.float64).contiguous()
        assert flat.shape == (self.num_envs, self.layout.export_width)
        check(self.lib.mate_engine_import_state(self._h, ctypes.c_void_p(flat.data_ptr()), self._stream()))
        torch.cuda.synchronize(self.device)

    def state_dict(self):
        """All state fields as numpy arrays [N, ...] (host copy)."""
        return self.state_dict_from(self.export_state().cpu().numpy())

    def load_state_dict(self, fields):
        flat = self.export_state().cpu().numpy()
        for name, value in fields.items():
            off, shape = self.export_fields[name]
            n = int(np.prod(shape)) if shape else 1
            flat[:, off:off + n] = np.asarray(value, dtype=np.float64).reshape(self.num_envs, n)
        self.import_state(torch.from_numpy(flat))

    def rebuild_luts(self):
        check(self.lib.mate_engine_rebuild_luts(self._h, self._stream()))

    def enable_outer_boundary(self):
        """Also build Camera.boundary_outer at every later reset / rebuild_luts (entities.py:419-448); needed only by
        boundary_between(outer=True)."""
        cap = ctypes.c_int32()
        check(self.lib.mate_engine_enable_outer_boundary(self._h, ctypes.byref(cap)))
        self.outer_capacity = cap.value

    def need_outer_boundary(self):
        """enable_outer_boundary() unless it is on already: built at every reset from now on, and once now for the running episodes."""
        if not self.outer_capacity:
            self.enable_outer_boundary()
            self.rebuild_luts()

    def lut_read(self, env, camera, outer=False):
        cap = self.outer_capacity if outer else self.layout.lut_capacity
        phis, rhos = np.zeros(cap), np.zeros(cap)
        n = ctypes.c_int32()
        fn = self.lib.mate_engine_lut_read_outer if outer else self.lib.mate_engine_lut_read
        check(fn(self._h, int(env), int(camera), phis.ctypes.data_as(ctypes.c_void_p), rhos.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(n)))
        return phis[:n.value].copy(), rhos[:n.value].copy()

    def lut_write(self, env, camera, phis, rhos, outer=False):
        phis = np.ascontiguousarray(phis, dtype=np.float64)
        rhos = np.ascontiguousarray(rhos, dtype=np.float64)
        fn = self.lib.mate_engine_lut_write_outer if outer else self.lib.mate_engine_lut_write
        check(fn(self._h, int(env), int(camera), phis.ctypes.data_as(ctypes.c_void_p), rhos.ctypes.data_as(ctypes.c_void_p), len(phis)))

    def soft_coverage(self, masks=None):
        """AuxiliaryCameraRewards' soft coverage score of the current state (wrappers/auxiliary_camera_rewards.py:128-139,
        181-239): (score matrix [N, Nc, Nt], per-camera scores [N, Nc]) f64 on the GPU.  `masks` = packed masks of the
        step this follows (default: the engine's own output buffer).  Needs enable_outer_boundary() + a reset /
        rebuild_luts since."""
        masks = self.masks if masks is None else masks
        assert masks.dtype == torch.int32 and masks.is_contiguous() and masks.shape == (self.num_envs, self.layout.mask_words)
        if self._softcov is None:
            self._softcov = (torch.empty((self.num_envs, self.num_cameras, self.num_targets), dtype=torch.float64, device=self.device),
                             torch.empty((self.num_envs, self.num_cameras), dtype=torch.float64, device=self.device))
        matrix, scores = self._softcov
        check(self.lib.mate_engine_soft_coverage(self._h, masks.data_ptr(), matrix.data_ptr(), scores.data_ptr(), self._stream()))
        return matrix, scores

    def idle_steps(self):
        """(environment, step) slots spent idle waiting for a batched reset since creation."""
        total = ctypes.c_int64()
        check(self.lib.mate_engine_idle_steps(self._h, ctypes.byref(total)))
        return total.value

    def snapshot_episode_stats(self, out):
        """`out` (5 f64 on the device) <- the episode-statistics accumulators, ordered on the current stream behind the launches enqueued
        so far (mate_engine_snapshot_episode_stats: one tiny launch)."""
        check(self.lib.mate_engine_snapshot_episode_stats(self._h, ctypes.c_void_p(out.data_ptr()), self._stream()))
        return out

    def set_sub_wave(self, enable='auto'):
        """Environments per wave of the fused rollouts (mate_engine_set_sub_wave): the small scenarios (at most four cameras and four
        targets) can step four environments per wave.  'auto' (the default of a new engine) = where that measured faster (batches of at
        least 32 environments per compute unit; under the random policy every such shape but MATE-4v4-*), True = in every fused
        launch of such a shape, False = one per wave.  Returns the number the Greedy rollouts now run with."""
        in_use = ctypes.c_int32()
        check(self.lib.mate_engine_set_sub_wave(self._h, 2 if enable == 'auto' else int(bool(enable)), ctypes.byref(in_use)))
        return in_use.value

    @property
    def sub_wave(self):
        """Environments per wave the fused Greedy rollouts run with (1, or 4 for the small scenarios)."""
        in_use = ctypes.c_int32()
        check(self.lib.mate_engine_set_sub_wave(self._h, -1, ctypes.byref(in_use)))
        return in_use.value

    def kernel_time(self, enable=1):
        """(avg ms, launches) of the step kernel since the last call; `enable` = k arms the HIP-event timer
        for every k-th launch (0 disarms)."""
        avg, n = ctypes.c_double(), ctypes.c_int64()
        check(self.lib.mate_engine_kernel_time(self._h, int(enable), ctypes.byref(avg), ctypes.byref(n)))
        return avg.value, n.value

    @property
    def last_flow(self):
        """Compilation of the step kernel the last launch ran: 0 generic, 1 random-policy flow, 2 f32-actions flow."""
        return int(self.lib.mate_engine_last_flow(self._h))

    # decoded masks ------------------------------------------------------------
    def unpack_masks(self, masks=None, words_host=None):
        """Packed u32 words -> dict of boolean numpy arrays [N, ...] (environment.py:475-494 names).  `words_host`: the words as a
        NumPy array already on the host (fetch_host)."""
        words = (words_host if words_host is not None else (self.masks if masks is None else masks).cpu().numpy()).astype(np.uint32)
        N, Nc, Nt, No = self.num_envs, self.num_cameras, self.num_targets, self.num_obstacles
        bits = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(N, -1)
        L = self.layout
        NJ = Nc + No + Nt
        ct = bits[:, L.bit_camera_target:L.bit_camera_target + Nc * Nt].reshape(N, Nc, Nt)
        cc = bits[:, L.bit_camera_camera:L.bit_camera_camera + Nc * Nc].reshape(N, Nc, Nc)
        rows = bits[:, L.bit_target_row:L.bit_target_row + Nt * NJ].reshape(N, Nt, NJ)
        co = np.zeros((N, Nc, No), dtype=bool)
        for c in range(Nc):
            co[:, c] = bits[:, L.bit_camera_obstacle + 64 * c:L.bit_camera_obstacle + 64 * c + No]
        return {
            'camera_target_view_mask': ct, 'camera_camera_view_mask': cc,
            'target_camera_view_mask': rows[:, :, :Nc], 'target_obstacle_view_mask': rows[:, :, Nc:Nc + No],
            'target_target_view_mask': rows[:, :, Nc + No:], 'camera_obstacle_view_mask': co,
            'tracked_bits': ct.any(axis=1),
        }


class Stepper:
    """The learner-in-the-loop stepping flow: `between()` (the caller's policy: any torch code that rewrites the joint
    action tensors in place) then `step((cam_act, tgt_act))`, with outputs in the engine's own observation / scalar /
    mask tensors.  With `graph_steps` = K > 0 the step counter moves to the device (Engine.device_tick) and K
    iterations are captured once in a HIP graph (torch.cuda.CUDAGraph: the policy's kernels and the engine's launches
    in one graph); `run(n)` replays it n // K times and launches the remainder directly.  The host then spends one
    graph launch per K steps instead of two kernel launches through ctypes per step.  Bit-identical to calling
    Engine.step in a loop (tested).  `close()` gives the step counter back to the host; an open reset interval (run()
    stopped between two reset launches) is closed there: what had finished in it restarts at once.

    NOTE -- building a graph Stepper ADVANCES the environments: before the capture, one whole reset interval
    (`auto_reset` real steps: `between()`, the greedy opponents of `versus`, the step) runs directly, so that every code
    object is loaded and the device-resident counter sits on an interval boundary.  Those `warmup_steps` transitions are
    real (outputs in the engine's tensors, episode statistics counted) and a learner that must see every transition
    reads them like any other step; "bit-identical to Engine.step in a loop" means a loop that includes them."""

    def __init__(self, eng, cam_act, tgt_act, auto_reset=True, graph_steps=0, between=None, versus=None, frame_skip=1):
        self.eng, self.between, self.graph_steps = eng, between, int(graph_steps)
        self.graph = None                                 # (set first: close() reads it, also of a stepper whose construction was refused)
        # frame_skip = K > 1 (with `versus`): FrameSkip(K) over MultiCamera / MultiTarget, the example trainers' flow -- every "step" of
        # this stepper is ONE K-frame launch (Engine.rollout_versus_greedy: the caller's action repeated, the greedy opponents acting
        # anew on every frame), `auto_reset` and `graph_steps` count launches, and run() returns the rollout-shaped tensors
        # ([K, N, ...]: the caller sums the reward rows, reads the last frame's observation) instead of the engine's per-step ones
        self.frame_skip = int(frame_skip)
        assert self.frame_skip >= 1 and (self.frame_skip == 1 or versus is not None), 'frame_skip belongs to the learner-versus-greedy flow'
        # per-frame fragments attached for `versus` (Engine.enable_fragment_rows(per_frame=True)): every "step" of this stepper is K per-step calls with the
        # action held, each followed by the frame launch -- any opponent; auto_reset counts ENGINE calls and is a multiple of K, graphs hold whole intervals
        self.per_frame = eng.fragment_per_frame and versus in (('camera', 'target')[eng.fragment_team], eng.fragment_team)
        if self.per_frame:
            assert self.frame_skip == eng.fragment_frame_skip, f'per-frame fragments of {eng.fragment_frame_skip} frames are attached: frame_skip must be that'
            if auto_reset is True:
                auto_reset = self.frame_skip
            assert int(auto_reset) >= 1 and int(auto_reset) % self.frame_skip == 0, 'per-frame fragments: auto_reset (engine calls) is a positive multiple of frame_skip'
        fused = self.frame_skip > 1 and not self.per_frame
        if fused and versus in ('camera', 0) and eng.target_agent != 'greedy':
            raise ValueError(f"make_stepper(versus='camera', frame_skip={self.frame_skip}) is one fused K-frame launch, which holds the Greedy agents: the target opponent is "
                             f"{eng.target_agent!r} (Engine.set_target_opponent) -- step per frame (frame_skip=1) or select 'greedy'")
        if fused and versus in ('target', 1) and eng.camera_agent != 'greedy' and eng.num_cameras > 0:
            raise ValueError(f"make_stepper(versus='target', frame_skip={self.frame_skip}) is one fused K-frame launch, which holds the Greedy agents: the camera opponent is "
                             f"{eng.camera_agent!r} (Engine.set_camera_opponent) -- step per frame (frame_skip=1) or select 'greedy'")
        for team, name in ((1, 'camera'), (0, 'target')):      # (the team the ENGINE plays against the learner `name`)
            if fused and versus in (name, 1 - team) and eng.mixtures[team] is not None and set(eng.mixtures[team]) != {'greedy'} and (team == 1 or eng.num_cameras > 0):
                raise ValueError(f"make_stepper(versus={name!r}, frame_skip={self.frame_skip}) is one fused K-frame launch, which holds the Greedy agents: the opponents play the mixture "
                                 f"{eng.mixtures[team]} (Engine.set_opponent_mixture) -- step per frame (frame_skip=1) or clear the mixture")
        for team, name in ((1, 'camera'), (0, 'target')):
            if fused and versus in (name, 1 - team) and eng.channels[team] is not None and (team == 1 or eng.num_cameras > 0):
                raise ValueError(f"make_stepper(versus={name!r}, frame_skip={self.frame_skip}) is one fused K-frame launch, which delivers every message: the opponents' team has the "
                                 f"communication channel {eng.channels[team]} (Engine.set_channel) -- step per frame (frame_skip=1) or clear the channel")
        self.auto_reset = int(auto_reset)        # True / 1: immediate; k > 1: batched (finished environments idle up to k - 1 steps)
        # versus = 'camera' / 'target': the caller's team (MultiCamera / MultiTarget); the other team is played by the on-device
        # greedy agents (Engine.step_versus_greedy) and its tensor argument is ignored
        # versus = 'selection': the camera learner emits target selections (Engine.enable_selection first); every step of this stepper is
        # one FRAGMENT of HierarchicalCamera: frame_skip x (executor, greedy targets + step, reward rows, metrics) with the selection held.
        # A finished environment must execute no further frame of its fragment and restart behind it: the frames run under the engine's
        # batched restart with the interval frame_skip (finished environments idle, done = 2; the restart, the action mask and the state
        # rows follow the fragment's LAST frame), and fragments stay aligned with that interval because (a) a fragment is only ever run
        # whole (_one), (b) the constructor closes whatever interval was open (device_tick on / off: what had finished restarts, the
        # count starts at 0) and (c) `auto_reset` must be 1 fragment.  Metrics, frames and accumulating reward rows are zeroed at the
        # head of every fragment, inside the graph too.
        # versus = 'seat': the learner's seat among on-device teammates (Engine.enable_seat first); the seat team's tensor argument is the seat's
        # action ([N, 2] or [N] grid indices), the other is ignored.  frame_skip = K: K per-step calls with the action held (there is no fused K-frame
        # seat flow), under the engine's batched restart with the interval K -- auto_reset must be K: a finished environment idles to its fragment's end
        self.seat = versus == 'seat'
        if self.seat:
            assert eng.seat_obs is not None, 'Engine.enable_seat() first'
            assert self.frame_skip == 1 or self.auto_reset == self.frame_skip, "versus='seat', frame_skip = K: auto_reset = K (finished environments restart behind their fragment)"
            seat_action = tgt_act if eng.seat_team == 1 else cam_act
            versus, cam_act, tgt_act = None, None, None
        self.selection = versus == 'selection'
        if self.selection:
            assert eng.selection is not None, 'Engine.enable_selection() first'
            assert self.auto_reset == 1, "versus='selection': finished environments restart behind their fragment (auto_reset = True)"
            assert self.frame_skip == 1 or eng.selection_accumulate, 'frame_skip > 1 sums the metrics over the frames: enable_selection(accumulate=True)'
            versus, cam_act, tgt_act = None, None, None
        self.versus = None if versus is None else _team_code(versus)
        if self.versus == 0:
            tgt_act = None
        elif self.versus == 1:
            cam_act = None
        self.io, self.keep = eng._seat_io(seat_action) if self.seat else eng._io(cam_act, tgt_act)
        assert not self.seat or getattr(self.io, ('camera', 'target')[eng.seat_team] + '_actions_dev') == seat_action.data_ptr(), 'the seat\'s action tensor must be contiguous on the engine device'
        # _io may have made contiguous copies: the stepper must read the caller's own storage
        assert (tgt_act is None or self.io.target_actions_dev == tgt_act.data_ptr()) and \
            (cam_act is None or eng.num_cameras == 0 or self.io.camera_actions_dev == cam_act.data_ptr()), \
            'action tensors must be contiguous f32/f64 (or int32 grid indices) on the engine device'
        self.outputs = None
        if self.frame_skip > 1 and not self.selection and not self.seat and not self.per_frame:
            # (the reward launch reads the last frame's masks; the fragment launch every frame's, for a mask term)
            shaped = eng.reward_coefficients is not None or (eng._fragment_masks and eng.fragment_team == self.versus) or eng._info_attached()
            buf = eng.reserve_rollout(self.frame_skip, want_masks=shaped)
            eng._bind_outputs(self.io, buf['camera_obs'], buf['target_obs'], buf['scalars'], buf['masks'] if shaped else None)
            self.outputs = (buf['camera_obs'][:self.frame_skip], buf['target_obs'][:self.frame_skip], buf['scalars'][:self.frame_skip])
            self.keep = (self.keep, buf)
        self.ref = ctypes.byref(self.io)
        self._phase = 0                                   # steps into the current reset interval (graphs hold whole intervals)
        self._interval = 1 if self.seat and self.frame_skip > 1 else self.auto_reset // self.frame_skip if self.per_frame else self.auto_reset      # _one() calls per reset interval (a seat fragment is a whole one)
        self.warmup_steps = self._interval if self.graph_steps > 0 else 0      # real steps the constructor runs (see the class note)
        if self.selection and self.frame_skip > 1:
            eng.device_tick(self.frame_skip)              # (closes an open reset interval: fragments start on an interval boundary)
            if self.graph_steps == 0:
                eng.device_tick(False)
        if self.graph_steps > 0:
            assert self.auto_reset >= 1 and self.graph_steps % self._interval == 0, \
                'graph replay needs auto_reset >= 1 (the auto-reset launch advances the device step counter) and whole reset intervals per graph'
            eng.device_tick(self.frame_skip if self.selection else self.auto_reset)
            for _ in range(self._interval):
                self._one()                               # code objects loaded before the capture (one whole reset interval)
            torch.cuda.synchronize(eng.device)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                for _ in range(self.graph_steps):
                    self._one()

    def _one(self):
        if self.between is not None:
            self.between()
        eng = self.eng
        if self.selection:
            if eng.selection_accumulate:
                eng.selection_metrics.zero_()
                eng.selection_frames.zero_()
                if eng.reward_coefficients is not None and eng.reward_accumulate:
                    for rows in (eng.camera_reward_rows, eng.target_reward_rows):
                        if rows is not None:
                            rows.zero_()
            status = 0
            for _ in range(self.frame_skip):
                status = status or eng.lib.mate_engine_step_selected(eng._h, self.ref, None, self.frame_skip if self.frame_skip > 1 else self.auto_reset, eng._stream())
        elif self.seat:
            status = 0
            for _ in range(self.frame_skip):
                status = status or eng.lib.mate_engine_step_seated(eng._h, self.ref, None, self.auto_reset, eng._stream())
        elif self.per_frame:
            status = 0
            for _ in range(self.frame_skip):
                status = status or eng.lib.mate_engine_step_versus_greedy(eng._h, self.versus, self.ref, None, self.auto_reset, eng._stream())
        elif self.versus is None:
            status = eng.lib.mate_engine_step(eng._h, self.ref, self.auto_reset, eng._stream())
        elif self.frame_skip > 1:
            status = eng.lib.mate_engine_rollout_versus_greedy(eng._h, self.versus, self.ref, self.frame_skip, self.auto_reset, eng._stream())
        else:
            status = eng.lib.mate_engine_step_versus_greedy(eng._h, self.versus, self.ref, None, self.auto_reset, eng._stream())
        if status != 0:
            check(status)

    def run(self, steps):
        steps = int(steps)
        if self.graph is not None:
            while steps > 0 and self._phase != 0:         # finish a reset interval a previous call stopped in, launch by launch
                self._one()
                self._phase = (self._phase + 1) % self._interval
                steps -= 1
            while steps >= self.graph_steps:              # whole graphs (whole reset intervals)
                self.graph.replay()
                steps -= self.graph_steps
            self._phase = steps % self._interval
        for _ in range(steps):
            self._one()
        if self.outputs is not None:
            return self.outputs
        eng = self.eng
        return eng.camera_obs, eng.target_obs, eng.scalars

    @property
    def state(self):
        """The engine's state rows ([N, state_dim]) when it has them attached (Engine.enable_state_rows BEFORE the stepper is built, so
        that the captured intervals contain the launch): the same tensor, refreshed by every step and every replay; else None."""
        return self.eng.state

    # The engine's shaped reward rows when it has them attached (Engine.enable_reward_rows BEFORE the stepper is built, so that the
    # captured intervals contain the launches): the same tensors, rewritten (or, accumulating, added to) by every step and every replay.
    camera_reward_rows = property(lambda self: self.eng.camera_reward_rows)
    target_reward_rows = property(lambda self: self.eng.target_reward_rows)
    camera_reward_terms = property(lambda self: self.eng.camera_reward_terms)
    target_reward_terms = property(lambda self: self.eng.target_reward_terms)
    reward_coefficients = property(lambda self: self.eng.reward_coefficients)
    # The engine's fragment tensors (Engine.enable_fragment_rows BEFORE the stepper is built: versus = that team, frame_skip = K): a dict
    # {'obs', 'rewards', 'done', 'frames', 'info', 'shaped', 'coefficients'} (+ 'first_rows', 'first_scalars', 'final_obs' with first_rows=True: the memset
    # node and the two launches behind the restart are captured with the rest), rewritten by every K-frame launch and every replay.
    fragment = property(lambda self: self.eng.fragment)

    def close(self):
        if self.graph is not None:
            torch.cuda.synchronize(self.eng.device)
            self.graph = None
            self._phase = 0
            self.eng.device_tick(False)                   # (closes an open reset interval: mate_engine_device_tick)

    def __del__(self):
        try:
            self.close()
        except Exception as exc:      # an engine left in device-tick mode refuses rollouts / seed / import_state: say so
            warnings.warn(f'Stepper.close() failed while the stepper was collected: {exc!r}; the engine may still count steps on the device', RuntimeWarning)


class EngineGroups:
    """One batch of N environments as G groups of N / G on G streams, for a learner that interleaves its groups (double-buffered
    sampling: while it computes the actions of one group, the other group steps).

    A one-launch-per-step flow leaves the GPU idle at every kernel boundary -- the tail of step t's slowest waves, the ramp of step
    t + 1, the caller's policy kernel in between, and the two dependency gaps around it: at 4096 x MATE-4v8-9 5 of a step's 14.5 us.
    Two independent half-batches on two streams fill each other's gaps: 14.5 -> 13.2 us per step of the whole batch at 4096
    environments, 33.7 -> 27.6 at 16 384 (+20 %; 0.456 -> 0.55 of the HBM roofline), 53.6 -> 43.8 for the learner-versus-greedy step;
    three groups do no better, four worse (profiles/r05_groups_probe.txt).  The groups ARE the batch: group g holds the global
    environment indices [first_env_index + g N / G, ...), so every environment's episode is, bit for bit, what the single engine of N
    steps (the random streams are keyed by the global index; tests/test_gpu_groups.py).

    `streams[0]` is the stream current at construction, the others come from `pick_streams()`: HIP maps streams onto a handful of
    hardware queues, and two streams that share a queue run their work one after the other (23 instead of 13 us per step when
    that happens) -- a short trial of a few fresh streams with the caller's own loop body picks ones that overlap."""

    def __init__(self, config, num_envs, groups=2, device=0, seed=0, first_env_index=0, obs_dtype=torch.float32, policies=False):
        assert groups >= 1 and num_envs % groups == 0, 'the groups share the batch evenly'
        self.groups, self.per_group = int(groups), int(num_envs) // int(groups)
        self.device = torch.device('cuda', int(device))
        self.streams = [torch.cuda.current_stream(self.device)] + [torch.cuda.Stream(device=self.device) for _ in range(self.groups - 1)]
        self.engines = []
        for g in range(self.groups):
            with torch.cuda.stream(self.streams[g]):
                eng = Engine(config, self.per_group, device=device, seed=seed, first_env_index=first_env_index + g * self.per_group, obs_dtype=obs_dtype)
                if policies:
                    eng.enable_policies()
                self.engines.append(eng)

    def each(self, fn):
        """fn(group index, engine) for every group, with the group's stream current; returns the results."""
        out = []
        for g, eng in enumerate(self.engines):
            with torch.cuda.stream(self.streams[g]):
                out.append(fn(g, eng))
        return out

    def reset(self):
        return self.each(lambda g, eng: eng.reset())

    def enable_state_rows(self, normalize=False, dtype=None):
        """Engine.enable_state_rows on every group, each on its own stream; returns the groups' state tensors (group g holds the rows
        of the global environments [g N / G, (g + 1) N / G))."""
        return self.each(lambda g, eng: eng.enable_state_rows(normalize=normalize, dtype=dtype))

    def enable_info_rows(self, camera=True, target=True, cargo=True):
        """Engine.enable_info_rows on every group, each on its own stream; returns the groups' (camera, target, cargo) row tensors."""
        return self.each(lambda g, eng: eng.enable_info_rows(camera=camera, target=target, cargo=cargo))

    def enable_fragment_rows(self, team, frame_skip, **kwargs):
        """Engine.enable_fragment_rows (per_frame=True included) on every group; returns the groups' fragment_obs tensors."""
        return self.each(lambda g, eng: eng.enable_fragment_rows(team, frame_skip, **kwargs))

    def step_fragment_frames(self, team, joint_actions, auto_reset=None):
        """Engine.step_fragment_frames on every group, each on its own stream (`joint_actions`: one tensor per group); returns the groups' fragment dicts."""
        return self.each(lambda g, eng: eng.step_fragment_frames(team, joint_actions[g], auto_reset=auto_reset))

    def disable_fragment_rows(self):
        return self.each(lambda g, eng: eng.disable_fragment_rows())

    def keep_masks(self):
        return self.each(lambda g, eng: eng.keep_masks())

    def render(self, envs=None, size=800, headings=None):
        """Engine.render of the batch's environments `envs` (indices into the WHOLE batch; None: all of them), each drawn by its group's engine on its
        group's stream into a tensor of that stream; the groups' streams are waited for, then ONE uint8 [k, size, size, 3] tensor in the order of `envs` is
        put together on the current stream.  The groups' engines need their own mask words (keep_masks(), or policies=True)."""
        index = np.arange(self.groups * self.per_group) if envs is None else np.asarray(envs, dtype=np.int64).reshape(-1)
        if index.size < 1 or index.min() < 0 or index.max() >= self.groups * self.per_group:
            raise ValueError(f'render: the environments must be indices in [0, {self.groups * self.per_group}) and at least one')
        headings = None if headings is None else np.asarray(torch.as_tensor(headings).cpu(), dtype=np.float64).reshape(index.size, -1)

        def draw(g, eng):      # (everything a group touches -- indices, headings, frames -- is allocated and uploaded on the group's own stream)
            mine = np.flatnonzero(index // self.per_group == g)
            return mine, (eng.render(index[mine] - g * self.per_group, size=size, headings=None if headings is None else headings[mine]) if mine.size else None)
        parts = self.each(draw)
        self.synchronize()
        out = torch.empty((index.size, int(size), int(size), 3), dtype=torch.uint8, device=self.device)
        for mine, frames in parts:
            if frames is not None:
                out[torch.from_numpy(mine).to(self.device)] = frames
        return out

    def enable_communication_trace(self, teams=('camera', 'target'), duration=20):
        """Engine.enable_communication_trace on every group."""
        return self.each(lambda g, eng: eng.enable_communication_trace(teams=teams, duration=duration))

    def communication_trace(self, team):
        """Engine.communication_trace of every group: the groups' [N / G, n, n] views."""
        return self.each(lambda g, eng: eng.communication_trace(team))

    def enable_messages(self, team, width, pairwise=False, addressed=False):
        """Engine.enable_messages on every group; returns the groups' (payload, address, inbox) tensors."""
        return self.each(lambda g, eng: eng.enable_messages(team, width, pairwise=pairwise, addressed=addressed))

    def route_messages(self, teams=None, round=0):
        """Engine.route_messages on every group, each on its own stream; returns the groups' inboxes."""
        return self.each(lambda g, eng: eng.route_messages(teams, round))

    def message_edges(self, team):
        return self.each(lambda g, eng: eng.message_edges(team))

    def message_tape(self, camera_u=None, target_u=None, record=False):
        """Engine.message_tape on every group (`camera_u` / `target_u`: None, or one tensor per group); returns the groups' records."""
        pick = lambda value, g: None if value is None else value[g]      # noqa: E731
        return self.each(lambda g, eng: eng.message_tape(pick(camera_u, g), pick(target_u, g), record=record))

    def synchronize(self):
        for s in self.streams:
            s.synchronize()

    def pick_streams(self, body, candidates=3, warm=2, timed=4):
        """Choose the side streams by trial.  `body(g, engine)` enqueues one slice of the caller's loop for group g (e.g. a Stepper
        replay); for every side stream, `candidates` fresh streams are tried with `warm + timed` rounds of all groups and the
        fastest is kept.  Returns the trial times [s] of the last group's candidates.

        The trial STEPS the environments (`candidates * (warm + timed)` slices per group): call it before the episodes that matter,
        or reset afterwards.  A group's engine moves to a stream that knows nothing of the work queued on its previous one (a
        reset, an import), so the device is synchronised before the first trial and at every change of stream; the engine's buffers
        were allocated on the first stream and live as long as the engine, so the caching allocator never hands them out again."""
        times = []
        torch.cuda.synchronize(self.device)           # everything queued on the groups' present streams is complete before one of them changes
        for g in range(1, self.groups):
            times = []
            pool = [torch.cuda.Stream(device=self.device) for _ in range(candidates)]
            for cand in pool:
                torch.cuda.synchronize(self.device)
                self.streams[g] = cand
                for _ in range(warm):
                    self.each(body)
                torch.cuda.synchronize(self.device)
                t0 = time.perf_counter()
                for _ in range(timed):
                    self.each(body)
                torch.cuda.synchronize(self.device)
                times.append(time.perf_counter() - t0)
            torch.cuda.synchronize(self.device)
            self.streams[g] = pool[times.index(min(times))]
        return times

    def idle_steps(self):
        return sum(eng.idle_steps() for eng in self.engines)

    def close(self):
        for eng in self.engines:
            eng.close()
