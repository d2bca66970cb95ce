"""The environment boundary: `MultiAgentTracking` (one environment, NumPy in/out -- the drop-in for
the reference class mate/environment.py:288) and `BatchedMultiAgentTracking` (N environments,
torch tensors resident in HBM).  Both are thin hosts over the HIP engine (`mate_amd.engine.Engine`);
there is no CPU simulation path in this package.
"""
import copy
from collections import OrderedDict, defaultdict, deque

import numpy as np
import torch

from mate_amd import constants as consts
from mate_amd import spaces
from mate_amd.auxiliary_rewards import CAMERA_REWARD_KEYS, AuxiliaryTargetRewards, reward_coefficient_table
from mate_amd.config import DEFAULT_CONFIG_FILE, read_config
from mate_amd.engine import CAMERA_AGENTS, SCALAR_NAMES, SCRIPTED_AGENTS, TARGET_AGENTS, Engine, channel_table, fragment_coefficient_table, mixture_table, seat_mode_of
from mate_amd.utils import Message, Team, arctan2_deg, normalize_angle, polar2cartesian

__all__ = ['MultiAgentTracking', 'BatchedMultiAgentTracking', 'EnvMeta']

try:  # reference wrappers are gym.Wrapper subclasses; inherit from gym.Env when gym exists
    import gym as _gym
    _EnvBase = _gym.Env
except Exception:  # pragma: no cover
    _gym = None

    class _EnvBase:
        metadata = {'render.modes': []}
        reward_range = (-float('inf'), float('inf'))
        spec = None

        @property
        def unwrapped(self):
            return self

        def __str__(self):
            return f'<{type(self).__name__}<{getattr(self.spec, "id", "MultiAgentTracking-v0")}>>'


class EnvMeta(type(_EnvBase)):
    """isinstance(wrapped_env, MultiAgentTracking) looks through wrapper chains (environment.py:272-284)."""

    def __instancecheck__(cls, instance):
        if super().__instancecheck__(instance):
            return True
        while hasattr(instance, 'env') and not super().__instancecheck__(instance):
            instance = instance.env
        return super().__instancecheck__(instance)


# --------------------------------------------------------------------------------------------- entity views
def _names_of(mixture):
    """The candidates with positive weight of a mixture given as a name, a sequence of names or a dict name -> weight (None: none)."""
    if mixture is None:
        return ()
    if isinstance(mixture, str):
        return (mixture,)
    if isinstance(mixture, dict):
        return tuple(name for name, w in mixture.items() if w > 0.0)
    return tuple(mixture)


class _EntityView:
    """Read-only window onto one entity of one environment (the reference exposes live objects)."""

    def __init__(self, env, index):
        self._env, self.index = env, index

    def _f(self, name):
        return self._env._fields()[name]

    @property
    def x(self):
        return self.location[0]

    @property
    def y(self):
        return self.location[1]

    def distance(self, other):
        other = other.location if isinstance(other, _EntityView) else np.asarray(other, dtype=np.float64)
        return float(np.linalg.norm(self.location - other))

    def __sub__(self, other):
        return self.location - other.location


class ObstacleView(_EntityView):
    @property
    def location(self):
        return np.array([self._f('obs_x')[self.index], self._f('obs_y')[self.index]])

    @property
    def radius(self):
        return float(self._f('obs_radius')[self.index])

    @property
    def transmittance(self):
        return self._env.obstacle_transmittance

    def state(self, private=False):
        return np.append(self.location, self.radius).astype(np.float64)


class CameraView(_EntityView):
    @property
    def location(self):
        return np.array([self._f('cam_x')[self.index], self._f('cam_y')[self.index]])

    @property
    def radius(self):
        return float(self._env.config['camera']['radius'])

    @property
    def orientation(self):
        return float(self._f('cam_phi')[self.index])

    @property
    def viewing_angle(self):
        return float(self._f('cam_theta')[self.index])

    @property
    def min_viewing_angle(self):
        return float(self._env.camera_min_viewing_angle)

    @property
    def max_sight_range(self):
        return float(self._env.camera_max_sight_range)

    @property
    def rotation_step(self):
        return float(self._env.camera_rotation_step)

    @property
    def zooming_step(self):
        return float(self._env.camera_zooming_step)

    @property
    def area_product(self):
        return self.min_viewing_angle * self.max_sight_range ** 2

    @property
    def sight_range(self):
        return float(np.sqrt(self.area_product / self.viewing_angle))

    def state(self, private=False):
        out = np.concatenate([self.location, [self.radius], polar2cartesian(self.sight_range, self.orientation), [self.viewing_angle]])
        if private:
            out = np.append(out, [self.max_sight_range, self.rotation_step, self.zooming_step])
        return out.astype(np.float64)

    def _table(self, outer=False):
        engine = self._env.engine
        if outer:
            engine.need_outer_boundary()
        return engine.lut_read(0, self.index, outer=outer)

    def sight_range_at(self, angle, outer=False):
        """Camera.sight_range_at (entities.py:507-511): linear interpolation of the (outer) occlusion boundary."""
        phis, rhos = self._table(outer)
        return float(np.interp((angle + 180.0) % 360.0 - 180.0, phis, rhos))

    def boundary_between(self, angle_left, angle_right, outer=False):
        """Knots of the occlusion boundary inside a sector (entities.py:513-543); like the reference, the two end
        points are interpolated on the INNER boundary whichever table the knots come from."""
        assert 0.0 < angle_right - angle_left <= 360.0
        phis_all, rhos_all = self._table(outer)
        left = (angle_left + 180.0) % 360.0 - 180.0
        right = left + (angle_right - angle_left)
        if right <= 180.0:
            pick = (left < phis_all) & (phis_all < right)
            phis, rhos = phis_all[pick], rhos_all[pick]
        else:
            a = (left < phis_all) & (phis_all <= 180.0)
            b = (phis_all > -180.0) & (phis_all < right - 360.0)
            phis, rhos = np.concatenate([phis_all[a], phis_all[b]]), np.concatenate([rhos_all[a], rhos_all[b]])
        phis = np.concatenate([[left], phis, [right]])
        rhos = np.concatenate([[self.sight_range_at(left)], rhos, [self.sight_range_at(right)]])
        return phis.astype(np.float64), rhos.astype(np.float64)


class TargetView(_EntityView):
    @property
    def location(self):
        return np.array([self._f('tgt_x')[self.index], self._f('tgt_y')[self.index]])

    radius = consts.TARGET_RADIUS

    @property
    def capacity(self):
        return int(self._f('tgt_capacity')[self.index])

    @property
    def step_size(self):
        return self._env.target_step_size / self.capacity

    @property
    def sight_range(self):
        return float(self._env.target_sight_range)

    @property
    def is_colliding(self):
        return bool(self._f('tgt_colliding')[self.index])

    @property
    def goal_bits(self):
        return self._f('tgt_goal_bits')[self.index].astype(np.int64)

    @property
    def empty_bits(self):
        return self._f('tgt_empty_bits')[self.index].astype(bool)

    @property
    def is_loaded(self):
        return bool(self.goal_bits.any())

    def state(self, private=False):
        out = np.append(self.location, [self.sight_range, self.is_loaded])
        if private:
            out = np.concatenate([out, [self.step_size, self.capacity], self.goal_bits, self.empty_bits])
        return out.astype(np.float64)


# --------------------------------------------------------------------------------------------- shared host logic
class _ScenarioMixin:
    """Configuration-derived attributes shared by the single and the batched environment."""

    def _setup_scenario(self, config, kwargs):
        if config is None:
            config = {} if len(kwargs) > 0 else DEFAULT_CONFIG_FILE
        self.config = read_config(config, **kwargs)

    # properties with the reference's names (environment.py:1396-1560)
    name = property(lambda self: self.config['name'])
    max_episode_steps = property(lambda self: self.config['max_episode_steps'])
    camera_min_viewing_angle = property(lambda self: self.config['camera']['min_viewing_angle'])
    camera_max_sight_range = property(lambda self: self.config['camera']['max_sight_range'])
    camera_rotation_step = property(lambda self: self.config['camera']['rotation_step'])
    camera_zooming_step = property(lambda self: self.config['camera']['zooming_step'])
    target_step_size = property(lambda self: self.config['target']['step_size'])
    target_sight_range = property(lambda self: self.config['target']['sight_range'])
    num_cargoes_per_target = property(lambda self: self.config['num_cargoes_per_target'])
    targets_start_with_cargoes = property(lambda self: self.config.get('targets_start_with_cargoes', True))
    bounty_factor = property(lambda self: max(0.0, self.config.get('bounty_factor', 1.0)))
    obstacle_transmittance = property(lambda self: min(max(0.0, self.config.get('obstacle', {}).get('transmittance', 0.0)), 1.0))
    shuffle_entities = property(lambda self: self.config.get('shuffle_entities', True))
    num_warehouses = property(lambda self: consts.NUM_WAREHOUSES)
    high_capacity_target_split = property(lambda self: min(max(0.0, self.config.get('high_capacity_target_split', 0.5)), 1.0))
    num_high_capacity_targets = property(lambda self: int(self.num_targets * self.high_capacity_target_split))
    num_low_capacity_targets = property(lambda self: self.num_targets - self.num_high_capacity_targets)
    camera_observation_dim = property(lambda self: self.camera_observation_space.shape[-1])
    target_observation_dim = property(lambda self: self.target_observation_space.shape[-1])

    def _need_policies(self):
        if not self._policies_on:      # (enable_greedy_policies sets it)
            raise RuntimeError('enable_greedy_policies() must precede the reset() the agents first act on')

    def _setup_spaces(self):
        Nc, Nt, No = self.num_cameras, self.num_targets, self.num_obstacles

        def box(lo, hi):
            return spaces.Box(low=np.asarray(lo, dtype=np.float64), high=np.asarray(hi, dtype=np.float64), dtype=np.float64)

        if Nc > 0:
            rot, zoom = self.camera_rotation_step, self.camera_zooming_step
            self.camera_action_space = box([-rot, -zoom], [rot, zoom])
        else:
            self.camera_action_space = box([0.0, 0.0], [0.0, 0.0])
        # the reference merges per-target boxes with an element-wise min (environment.py:369-378):
        # with mixed capacities the joint bound is the full step size of a capacity-1 target
        step = self.target_step_size
        self.target_action_space = box([-step, -step], [step, step])
        self.camera_joint_action_space = spaces.Tuple((self.camera_action_space,) * Nc)
        self.target_joint_action_space = spaces.Tuple((self.target_action_space,) * Nt)
        self.action_space = spaces.Tuple((self.camera_joint_action_space, self.target_joint_action_space))
        self.camera_observation_space = consts.camera_observation_space_of(Nc, Nt, No)
        self.target_observation_space = consts.target_observation_space_of(Nc, Nt, No)
        self.camera_joint_observation_space = spaces.Tuple((self.camera_observation_space,) * Nc)
        self.target_joint_observation_space = spaces.Tuple((self.target_observation_space,) * Nt)
        self.observation_space = spaces.Tuple((self.camera_joint_observation_space, self.target_joint_observation_space))
        self.camera_state_space_public, self.camera_state_space_private = consts.CAMERA_STATE_SPACE_PUBLIC, consts.CAMERA_STATE_SPACE_PRIVATE
        self.target_state_space_public, self.target_state_space_private = consts.TARGET_STATE_SPACE_PUBLIC, consts.TARGET_STATE_SPACE_PRIVATE
        self.obstacle_state_space = consts.OBSTACLE_STATE_SPACE
        self.state_space = consts.state_space_of(Nc, Nt, No)
        self.freight_scale = float(np.ceil(consts.TERRAIN_WIDTH / self.target_step_size))
        self.bounty_scale = float(np.ceil(self.freight_scale * self.bounty_factor))
        self.reward_scale = self.freight_scale + self.bounty_scale
        self.max_target_team_episode_reward = self.reward_scale * self.num_cargoes_per_target * Nt


class MultiAgentTracking(_ScenarioMixin, _EnvBase, metaclass=EnvMeta):
    """One Multi-Agent Tracking environment on the MI355X engine, with the reference's Python API:
    `seed / reset / step / state / joint_observation / send_messages / receive_messages / load_config /
    close` and the attribute set its wrappers and harnesses read."""

    metadata = {'render.modes': ['human', 'rgb_array'], 'video.frames_per_second': 60, 'video.output_frames_per_second': 60}
    DEFAULT_CONFIG_FILE = DEFAULT_CONFIG_FILE

    def __init__(self, config=None, device=0, obs_dtype=torch.float64, no_communication='none', message_dropout=0.0, communication_range=None, **kwargs):
        # the reference's NoCommunication / RandomMessageDropout / RestrictedCommunicationRange wrappers for the step_greedy() path (Engine.set_channel;
        # DESIGN.md section 3.15): checked now, set by enable_greedy_policies
        self._channels = channel_table(no_communication, message_dropout, communication_range)
        self._setup_scenario(config, kwargs)
        self._device_index, self._obs_dtype = device, obs_dtype
        self._seed_value = 0
        self.engine = Engine(self.config, 1, device=device, seed=0, obs_dtype=obs_dtype)
        self.engine.keep_masks()             # (render() reads the engine's own mask words: kept from the first reset on)
        self.engine.stage_outputs()          # one device-to-host copy per step (Engine.fetch_host)
        Na = self.engine.num_cameras * consts.CAMERA_ACTION_DIM + self.engine.num_targets * consts.TARGET_ACTION_DIM
        self._act_dev = torch.zeros(Na, dtype=torch.float64, device=self.engine.device)      # ... and one host-to-device copy of the joint action,
        self._act_host = torch.zeros(Na, dtype=torch.float64, pin_memory=True)               # from page-locked memory
        self.num_cameras, self.num_targets, self.num_obstacles = self.engine.num_cameras, self.engine.num_targets, self.engine.num_obstacles
        self._setup_spaces()
        Nc, Nt, No = self.num_cameras, self.num_targets, self.num_obstacles
        self.cameras = [CameraView(self, c) for c in range(Nc)]
        self.targets = [TargetView(self, t) for t in range(Nt)]
        self.obstacles = [ObstacleView(self, o) for o in range(No)]
        self.cameras_ordered, self.targets_ordered, self.obstacles_ordered = list(self.cameras), list(self.targets), list(self.obstacles)
        self.preserved_data = np.concatenate([[Nc, Nt, No], [0], consts.WAREHOUSES.ravel(), [consts.WAREHOUSE_RADIUS]]).astype(np.float64)
        self._sparse_reward = self.config['reward_type'] == 'sparse'
        self.viewer = None
        self.render_callbacks = OrderedDict()
        self.camera_message_buffer, self.target_message_buffer = defaultdict(list), defaultdict(list)
        self.message_buffers = (self.camera_message_buffer, self.target_message_buffer)
        self.camera_message_queue, self.target_message_queue = defaultdict(deque), defaultdict(deque)
        self.message_queues = (self.camera_message_queue, self.target_message_queue)
        self.camera_communication_edges = np.zeros((Nc, Nc), dtype=np.int64)
        self.target_communication_edges = np.zeros((Nt, Nt), dtype=np.int64)
        self.camera_total_communication_edges = self.camera_communication_edges.copy()
        self.target_total_communication_edges = self.target_communication_edges.copy()
        self.communication_edges = (self.camera_communication_edges, self.target_communication_edges)
        self.coverage_rate = self.real_coverage_rate = self.mean_transport_rate = 0.0
        self.num_delivered_cargoes = 0
        self.episode_step = 0
        self._cache = self._masks = self._np_random = None
        self._policies_on = False                         # (enable_greedy_policies)
        self.target_dones, self._last_goals = np.zeros(Nt, dtype=bool), None                  # (reset, _finish_step)
        # render-only state the engine does not keep (environment.py:1347-1352 of the reference): kept here from consecutive locations
        self.target_orientations, self._last_locations = np.zeros(Nt, dtype=np.float64), None
        self._last_episode_rewards = self._last_step_rewards = (0.0, 0.0)
        self.render_communication_duration = 0            # (enable_render_communication)
        self.camera_comm_matrix, self.target_comm_matrix = np.zeros((Nc, Nc), dtype=np.int64), np.zeros((Nt, Nt), dtype=np.int64)
        self.seed(0)

    # ------------------------------------------------------------------ state access
    def _fields(self):
        if self._cache is None:
            self._cache = {k: v[0] for k, v in self.engine.state_dict().items()}
        return self._cache

    def _mask(self, name):
        if self._masks is None:
            self._masks = {k: v[0] for k, v in self.engine.unpack_masks().items()}
        return self._masks[name]

    camera_target_view_mask = property(lambda self: self._mask('camera_target_view_mask'))
    target_camera_view_mask = property(lambda self: self._mask('target_camera_view_mask'))
    target_obstacle_view_mask = property(lambda self: self._mask('target_obstacle_view_mask'))
    target_target_view_mask = property(lambda self: self._mask('target_target_view_mask'))
    camera_camera_view_mask = property(lambda self: self._mask('camera_camera_view_mask'))
    camera_obstacle_view_mask = property(lambda self: self._mask('camera_obstacle_view_mask'))
    tracked_bits = property(lambda self: self._mask('tracked_bits'))
    remaining_cargoes = property(lambda self: self._fields()['remaining_cargoes'].astype(np.int64))
    awaiting_cargo_counts = property(lambda self: self._fields()['awaiting_cargo_counts'].astype(np.int64))
    target_goals = property(lambda self: self._fields()['tgt_goals'].astype(np.int64))
    target_goal_bits = property(lambda self: self._fields()['tgt_goal_bits'].astype(np.int64))
    target_capacities = property(lambda self: self._fields()['tgt_capacity'].astype(np.int64))
    target_steps = property(lambda self: self._fields()['target_steps'].astype(np.int64))
    tracked_steps = property(lambda self: self._fields()['tracked_steps'].astype(np.int64))
    freights = property(lambda self: self._fields()['freights'].astype(np.int64))
    bounties = property(lambda self: self._fields()['bounties'].astype(np.int64))
    target_team_episode_reward = property(lambda self: float(self._fields()['episode_reward']))
    delayed_target_team_episode_reward = property(lambda self: float(self._fields()['delayed_episode_reward']))

    @property
    def obstacle_states(self):
        f = self._fields()
        return np.stack([f['obs_x'], f['obs_y'], f['obs_radius']], axis=-1).reshape(self.num_obstacles, 3)

    @property
    def obstacle_states_flagged(self):
        return np.hstack([self.obstacle_states, np.ones((self.num_obstacles, 1))])

    @property
    def target_warehouse_distances(self):
        f = self._fields()
        xy = np.stack([f['tgt_x'], f['tgt_y']], axis=-1)
        return np.linalg.norm(xy[:, None, :] - consts.WAREHOUSES[None], axis=-1)

    @property
    def np_random(self):
        if self._np_random is None:
            self.seed()
        return self._np_random

    # ------------------------------------------------------------------ gym API
    def seed(self, seed=None):
        """Seed the host RNG handed to callers and the engine's counter-based streams (environment.py:1203-1227).

        Returns the main seed followed by one seed per entity (cameras, targets, obstacles), drawn from the fresh main
        generator exactly as the reference draws them (`np_random.randint(int_max)` per entity), so `len(env.seed())`
        and the position of `env.np_random` afterwards match.  The engine itself needs one key: its streams are
        Philox counters keyed by (seed, environment, episode, tick), and seeding rewinds those counters, so the same
        seed always produces the same episodes -- like the reference, whose `__init__` also ends with `seed(0)`."""
        if seed is None:
            seed = int(np.random.SeedSequence().entropy % (2 ** 31))
        if not (isinstance(seed, (int, np.integer)) and seed >= 0):
            raise ValueError(f'Seed must be a non-negative integer or omitted, not {seed}')
        self._seed_value = int(seed)
        self._np_random = np.random.RandomState(self._seed_value % (2 ** 32))
        self._heading_random = np.random.RandomState(self._seed_value % (2 ** 32))      # (the headings of targets without a goal at reset: a stream of its own, np_random stays where the reference leaves it)
        self.engine.seed(self._seed_value)
        int_max = np.iinfo(int).max
        entities = self.num_cameras + self.num_targets + self.num_obstacles
        return [self._seed_value] + [int(self._np_random.randint(int_max)) for _ in range(entities)]

    def _collect(self):
        """Fresh observations + the metrics of joint_observation (environment.py:966-979), computed here in f64 from the
        exported state and masks as the reference computes them (the engine's own scalar record is f32: the batched
        product dtype)."""
        host = self.engine.fetch_host()
        self._cache = {k: v[0] for k, v in self.engine.state_dict_from(host['state']).items()}
        self._masks = {k: v[0] for k, v in self.engine.unpack_masks(words_host=host['masks']).items()}
        cam = host['camera_obs'][0].astype(np.float64) if self.num_cameras else np.zeros((0, self.camera_observation_dim))
        tgt = host['target_obs'][0].astype(np.float64)
        scalars = host['scalars'][0].copy()
        f = self._fields()
        tracked = self.tracked_bits.astype(bool)
        with_bounty = f['bounties'] > 0
        self.coverage_rate = tracked.sum() / self.num_targets
        self.real_coverage_rate = float(np.logical_and(tracked, with_bounty).sum() / max(1, with_bounty.sum())) if with_bounty.any() else 0.0
        self.coverage_rate = float(self.coverage_rate)
        self.num_delivered_cargoes = int(f['num_delivered_cargoes'])
        self.mean_transport_rate = (float(f['delayed_episode_reward']) / (self.reward_scale * self.num_delivered_cargoes)
                                    if self.num_delivered_cargoes > 0 else 0.0)
        return cam, tgt, scalars

    def enable_render_communication(self, duration=20):
        """mate.RenderCommunication(env, duration) for this class: the wrapper's two matrices, camera_comm_matrix / target_comm_matrix [n, n] int64
        ([sender][recipient]), kept on the host from message_buffers -- counted down and marked at every step(), ahead of the step, and cleared at reset(),
        as the wrapper does -- and uploaded for the launch by render(), which then draws the dashed arrows.  The messages are the
        host mailbox's (send_messages).  The on-device agents of step_greedy() / step_versus_greedy() send none through it: with enable_greedy_policies()
        ahead of this call the engine traces theirs itself (Engine.enable_communication_trace, which installs a transparent channel for a team without
        one), and render() draws the union -- the element-wise maximum, both count down alike.  duration: 1 .. 255; 0 disables."""
        duration = int(duration)
        if not 0 <= duration <= 255:
            raise ValueError(f'enable_render_communication: duration must lie in [1, 255] (0 disables), got {duration}')
        self.render_communication_duration = duration
        self.camera_comm_matrix.fill(0)
        self.target_comm_matrix.fill(0)
        teams = [t for t, n in (('camera', self.num_cameras), ('target', self.num_targets)) if n > 0] if duration else []
        self.engine.enable_communication_trace(teams=teams, duration=duration or 20, channels=self._policies_on)

    def _trace_messages(self):
        """RenderCommunication.step ahead of env.step (render_communication.py:47-54)."""
        if not self.render_communication_duration:
            return
        for matrix, buffer in zip((self.camera_comm_matrix, self.target_comm_matrix), self.message_buffers):
            np.maximum(matrix - 1, 0, out=matrix)
            for packs in buffer.values():
                for message in packs:
                    matrix[message.sender, message.recipient] = self.render_communication_duration

    def reset(self, *, seed=None):
        self.camera_comm_matrix.fill(0)
        self.target_comm_matrix.fill(0)
        self._clear_messages(totals=True)
        if seed is not None:
            self.seed(seed)
        self.engine.reset()
        cam, tgt, _ = self._collect()
        self.target_dones = np.zeros(self.num_targets, dtype=bool)
        self._last_goals = self.target_goals.copy()
        self._last_episode_rewards = (self.target_team_episode_reward, self.delayed_target_team_episode_reward)
        self.episode_step = 0
        self._last_locations = self._target_locations()
        for t, goal in enumerate(self._last_goals):      # environment.py:814-821: towards the goal, a random heading without one
            away = consts.WAREHOUSES[goal] - self._last_locations[t] if goal >= 0 else None
            self.target_orientations[t] = arctan2_deg(away[1], away[0]) if goal >= 0 else normalize_angle(360.0 * self._heading_random.random_sample())
        return cam, tgt

    def _target_locations(self):
        f = self._fields()
        return np.stack([f['tgt_x'], f['tgt_y']], axis=-1).reshape(self.num_targets, 2).astype(np.float64)

    #: parity hook: {'camera_target': [Nc, Nt] uniforms, 'goal': [Nt] uniforms} consumed by the NEXT step() instead of the
    #: engine's Philox draws (how the golden traces recorded from the reference are replayed through this API)
    step_tape = None

    def _tapes(self):
        tape, self.step_tape = self.step_tape, None
        if not tape:
            return None, None
        dev = self.engine.device
        ct = tape.get('camera_target')
        goal = tape.get('goal')
        ct = None if ct is None else torch.from_numpy(np.nan_to_num(np.asarray(ct, dtype=np.float64), nan=0.0)[None].copy()).to(dev)
        goal = None if goal is None else torch.from_numpy(np.nan_to_num(np.asarray(goal, dtype=np.float64), nan=0.0)[None].copy()).to(dev)
        return ct, goal

    def enable_greedy_policies(self, target_agent='greedy', camera_agent='greedy', target_mixture=None, camera_mixture=None):
        """Let the engine play GreedyCameraAgent vs GreedyTargetAgent itself (`step_greedy`); call before the reset()
        whose observations the agents first act on.  target_agent='heuristic': HeuristicTargetAgent plays the targets
        (Engine.set_target_opponent); camera_agent='heuristic': HeuristicCameraAgent the cameras (Engine.set_camera_opponent).
        target_mixture / camera_mixture: a name of SCRIPTED_AGENTS or a dict name -> weight, the per-episode opponent mixture of that
        team (Engine.set_opponent_mixture) in place of the plain agent."""
        mixtures = {team: mixture_table(spec) and spec for team, spec in (('target', target_mixture), ('camera', camera_mixture)) if spec is not None}
        self.engine.enable_policies(target_agent=target_agent, camera_agent=camera_agent)
        for team, spec in mixtures.items():
            self.engine.set_opponent_mixture(team, spec)
        for team, spec in enumerate(self._channels):
            if spec is not None:
                self.engine.set_channel(team, **spec)
        self._policies_on = True
        if self.render_communication_duration:      # (enabled ahead of the agents: the engine-played teams' transparent channels now)
            self.enable_render_communication(self.render_communication_duration)

    def communication_edges(self):
        """((camera sent, camera delivered), (target sent, target delivered)) of the last step_greedy() / step_versus_greedy(): [n, n] int8 arrays,
        [sender][recipient] -- what the on-device agents handed to their channel and what arrived (Engine.channel_edges)."""
        self._need_policies()
        return tuple(tuple(x[0].cpu().numpy() for x in self.engine.channel_edges(team)) for team in (0, 1))

    def step_greedy(self):
        """`env.step(mate.group_step(...))` of both teams with the reference's Greedy agents computed on the device
        (mate/agents/greedy.py through Engine.step_greedy); same return value as step()."""
        self._need_policies()
        self._trace_messages()
        tape_ct, tape_goal = self._tapes()
        self.engine.step_greedy(tape_ct=tape_ct, tape_goal=tape_goal, auto_reset=False)
        return self._finish_step()

    def step_versus_greedy(self, team, joint_action):
        """`mate.MultiCamera(env, target_agent=GreedyTargetAgent()).step(joint_action)` for team = 'camera' (or mate_amd.Team.CAMERA),
        `mate.MultiTarget(env, camera_agent=GreedyCameraAgent()).step(...)` for 'target' (mate/wrappers/single_team.py:245-264): the
        caller's team acts, the greedy opponents act on the device.  Same return value as step() (both teams' halves)."""
        self._need_policies()
        team = getattr(team, 'name', team)
        team = team.lower() if isinstance(team, str) else ('camera', 'target')[int(team)]
        assert team in ('camera', 'target'), f'Invalid team {team!r}.'
        agents, dim = (self.num_cameras, consts.CAMERA_ACTION_DIM) if team == 'camera' else (self.num_targets, consts.TARGET_ACTION_DIM)
        act = np.asarray(joint_action, dtype=np.float64).reshape(agents, dim)
        assert np.isfinite(act).all(), f'Got unexpected joint action {act}.'
        self._trace_messages()
        tape_ct, tape_goal = self._tapes()
        self.engine.step_versus_greedy(team, torch.from_numpy(act[None]).to(self.engine.device), tape_ct=tape_ct, tape_goal=tape_goal,
                                       auto_reset=False)
        return self._finish_step()

    def step(self, action):
        camera_joint_action, target_joint_action = action
        cam_act = np.asarray(camera_joint_action, dtype=np.float64).reshape(self.num_cameras, consts.CAMERA_ACTION_DIM)
        tgt_act = np.asarray(target_joint_action, dtype=np.float64).reshape(self.num_targets, consts.TARGET_ACTION_DIM)
        assert np.isfinite(cam_act).all(), f'Got unexpected joint action {cam_act}.'
        assert np.isfinite(tgt_act).all(), f'Got unexpected joint action {tgt_act}.'
        self._trace_messages()
        tape_ct, tape_goal = self._tapes()
        nc = cam_act.size
        act_np = self._act_host.numpy()
        act_np[:nc] = cam_act.ravel()
        act_np[nc:] = tgt_act.ravel()
        self._act_dev.copy_(self._act_host, non_blocking=True)      # (stream-ordered before the step; the next call rewrites the host buffer only after fetch_host's synchronise)
        self.engine.step(self._act_dev[:nc].view(1, self.num_cameras, consts.CAMERA_ACTION_DIM), self._act_dev[nc:].view(1, self.num_targets, consts.TARGET_ACTION_DIM),
                         tape_ct=tape_ct, tape_goal=tape_goal, auto_reset=False)
        return self._finish_step()

    def _finish_step(self):
        cam, tgt, scalars = self._collect()
        goals = self.target_goals
        self.target_dones = (goals != self._last_goals) & (self._last_goals >= 0)
        self._last_goals = goals.copy()
        self.episode_step += 1
        locations = self._target_locations()
        moved = locations - self._last_locations
        for t in np.flatnonzero((moved != 0.0).any(axis=-1)):      # environment.py:1347-1352
            self.target_orientations[t] = arctan2_deg(moved[t, 1], moved[t, 0])
        self._last_locations = locations
        # the step's team reward in f64: the increment of the episode sums (integers: exact), environment.py:618-624
        sums = (self.target_team_episode_reward, self.delayed_target_team_episode_reward)
        r_tgt = float(sums[1] - self._last_episode_rewards[1]) if self._sparse_reward else float(sums[0] - self._last_episode_rewards[0])
        self._last_step_rewards = (float(sums[0] - self._last_episode_rewards[0]), float(sums[1] - self._last_episode_rewards[1]))
        self._last_episode_rewards = sums
        assert np.float32(r_tgt) == scalars[1]
        r_cam = -r_tgt
        done = bool(scalars[2])
        norm = r_tgt / self.max_target_team_episode_reward
        common = {'coverage_rate': self.coverage_rate, 'real_coverage_rate': self.real_coverage_rate,
                  'mean_transport_rate': self.mean_transport_rate, 'num_delivered_cargoes': self.num_delivered_cargoes}
        camera_infos = [dict(raw_reward=r_cam, normalized_raw_reward=-norm, messages=self.camera_message_buffer[c],
                             out_communication_edges=self.camera_communication_edges[c, :].sum(),
                             in_communication_edges=self.camera_communication_edges[:, c].sum(), **common)
                        for c in range(self.num_cameras)]
        target_infos = [dict(raw_reward=r_tgt, normalized_raw_reward=norm, messages=self.target_message_buffer[t],
                             out_communication_edges=self.target_communication_edges[t, :].sum(),
                             in_communication_edges=self.target_communication_edges[:, t].sum(), **common)
                        for t in range(self.num_targets)]
        self._clear_messages(totals=False)
        return (cam, tgt), (r_cam, r_tgt), done, (camera_infos, target_infos)

    def snapshot(self):
        """Everything a caller of the reference class can read after reset() / step(), as one dict of NumPy values keyed
        like the golden fixtures (tests/golden): the backend protocol of mate_amd.reference_adapter."""
        f = self._fields()
        Nc, Nt, No = self.num_cameras, self.num_targets, self.num_obstacles
        area = self.config['camera']['min_viewing_angle'] * self.config['camera']['max_sight_range'] ** 2 if Nc else 0.0
        last = self._last_step_rewards
        snap = {
            'cam_xy': np.stack([f['cam_x'], f['cam_y']], axis=-1).reshape(Nc, 2), 'cam_phi': f['cam_phi'].copy(), 'cam_theta': f['cam_theta'].copy(),
            'cam_sight': np.sqrt(area / f['cam_theta']) if Nc else np.zeros(0),
            'obs_xyr': np.stack([f['obs_x'], f['obs_y'], f['obs_radius']], axis=-1).reshape(No, 3),
            'tgt_xy': np.stack([f['tgt_x'], f['tgt_y']], axis=-1).reshape(Nt, 2), 'tgt_capacity': f['tgt_capacity'].astype(np.int64),
            'tgt_colliding': f['tgt_colliding'].astype(bool), 'tgt_empty_bits': f['tgt_empty_bits'].astype(bool),
            'tgt_goal_bits': f['tgt_goal_bits'].astype(np.int64), 'tgt_goals': self.target_goals, 'freights': self.freights, 'bounties': self.bounties,
            'target_steps': self.target_steps, 'tracked_steps': self.tracked_steps, 'remaining_cargoes': self.remaining_cargoes,
            'awaiting_cargo_counts': self.awaiting_cargo_counts, 'num_delivered_cargoes': int(f['num_delivered_cargoes']),
            'target_warehouse_distances': self.target_warehouse_distances, 'target_dones': np.asarray(self.target_dones, dtype=bool),
            'coverage_rate': self.coverage_rate, 'real_coverage_rate': self.real_coverage_rate, 'mean_transport_rate': self.mean_transport_rate,
            'reward_dense': last[0], 'reward_delayed': last[1],
            'luts': [self.engine.lut_read(0, c) for c in range(Nc)],
        }
        for name in ('camera_target_view_mask', 'target_camera_view_mask', 'target_obstacle_view_mask', 'target_target_view_mask',
                     'camera_camera_view_mask', 'camera_obstacle_view_mask', 'tracked_bits'):
            snap[name] = self._mask(name).copy()
        return snap

    def joint_observation(self):
        self.engine.observe()
        cam, tgt, _ = self._collect()
        return cam, tgt

    def state(self):
        f = self._fields()
        parts = [self.preserved_data] + [c.state(private=True) for c in self.cameras] + [t.state(private=True) for t in self.targets] \
            + [o.state() for o in self.obstacles] + [f['freights'], f['bounties'], f['remaining_cargoes'].ravel()]
        return np.concatenate(parts).astype(np.float64)

    def load_config(self, config=None):
        seed = self.np_random.randint(np.iinfo(np.int32).max)
        self.engine.close()
        self.__init__(config=config, device=self._device_index, obs_dtype=self._obs_dtype)
        self.seed(seed)

    def render(self, mode='human', window_size=800, **kwargs):
        """mode='rgb_array': the picture of the current state, uint8 [window_size, window_size, 3] (row 0 at the top), rasterised on the device by
        Engine.render under the rules of DESIGN.md sections 3.20 and 3.21 -- the reference's display list without the warehouse icons and without the
        render callbacks, but for RenderCommunication's arrows after enable_render_communication().  mode='human' needs a window: there is no display on
        the GPU box."""
        if mode != 'rgb_array':
            raise NotImplementedError("only mode='rgb_array' is rendered (off-screen, on the device): there is no display on the GPU box")
        if self.render_communication_duration:
            episode = int(self._fields()['episode'])
            for team, matrix in enumerate((self.camera_comm_matrix, self.target_comm_matrix)):
                if matrix.size:
                    merged = matrix      # (the wrapper's matrices stay as step() left them: the union goes to the device only)
                    if int(self.engine.communication_trace_tags(team)[0]) == episode:      # (the engine's own trace of the on-device agents, where it is this episode's)
                        merged = np.maximum(matrix, self.engine.communication_trace(team)[0].cpu().numpy().astype(np.int64))
                    self.engine.set_communication_trace(team, merged.astype(np.uint8)[None])
        frames = self.engine.render([0], size=window_size, headings=self.target_orientations[None])
        return frames[0].cpu().numpy()

    def add_render_callback(self, name, callback):
        self.render_callbacks[name] = callback

    def close(self):
        self.engine.close()

    def __str__(self):
        def plural(n, word):
            return f'{n} {word}{"s" if n > 1 else ""}'
        return f'{_EnvBase.__str__(self)}({plural(self.num_cameras, "camera")}, {plural(self.num_targets, "target")}, {plural(self.num_obstacles, "obstacle")})'

    # ------------------------------------------------------------------ intra-team messaging (host-side mailbox)
    def _clear_messages(self, totals):
        if totals:
            self.camera_total_communication_edges.fill(0)
            self.target_total_communication_edges.fill(0)
        else:
            self.camera_total_communication_edges += self.camera_communication_edges
            self.target_total_communication_edges += self.target_communication_edges
        self.camera_communication_edges.fill(0)
        self.target_communication_edges.fill(0)
        for store in (self.camera_message_buffer, self.target_message_buffer, self.camera_message_queue, self.target_message_queue):
            store.clear()

    def route_messages(self, messages):
        """Expand broadcasts into one message per teammate (environment.py:1249-1269)."""
        routed = []
        for message in messages:
            if message.recipient is None:
                for recipient in range((self.num_cameras, self.num_targets)[message.team.value]):
                    routed.append(Message(sender=message.sender, recipient=recipient, content=copy.deepcopy(message.content),
                                          team=message.team, broadcasting=True))
            else:
                routed.append(message)
        return routed

    def send_messages(self, messages):
        if isinstance(messages, Message):
            messages = (messages,)
        messages = list(messages)
        assert len({m.team for m in messages}) <= 1, f'All messages must be from the same team. Got messages = {messages}.'
        for message in self.route_messages(messages):
            team = message.team.value
            self.message_queues[team][message.recipient].append(message)
            self.message_buffers[team][message.recipient].append(message)
            self.communication_edges[team][message.sender, message.recipient] += 1

    def receive_messages(self, agent_id=None, agent=None):
        if agent_id is None and agent is None:
            out = ([list(self.camera_message_queue[c]) for c in range(self.num_cameras)],
                   [list(self.target_message_queue[t]) for t in range(self.num_targets)])
            self.camera_message_queue.clear()
            self.target_message_queue.clear()
            return out
        if agent_id is not None and not isinstance(agent_id, tuple) and agent is None:
            agent_id, agent = None, agent_id
        team, index = (agent.TEAM, agent.index) if agent is not None else agent_id
        out = list(self.message_queues[team.value][index])
        del self.message_queues[team.value][index]
        return out


def fragment_arguments(config, frame_skip, learner, camera_reward_shaping=None, target_reward_shaping=None, enhanced_observation=None,
                       shared_field_of_view=None, camera_selection=None, target_agent='greedy', camera_agent='greedy', per_frame=False):
    """The argument rules of BatchedMultiAgentTracking(frame_skip=K, learner=...), checked ahead of everything that needs a GPU.
    Returns None without `frame_skip`, else {'frame_skip', 'learner', 'shaping'}: the learner's (coefficients, reduction) or None.
    `per_frame`: the fragments are built frame by frame behind K per-step calls -- any `target_agent` / `camera_agent`
    and every shaping term of the learner's team; the result then also says 'per_frame': True."""
    assert target_agent in TARGET_AGENTS, f'target_agent = {target_agent!r}: one of {TARGET_AGENTS}'
    assert camera_agent in CAMERA_AGENTS, f'camera_agent = {camera_agent!r}: one of {CAMERA_AGENTS}'
    if frame_skip is None:
        assert learner is None, "learner = ... belongs to frame_skip = K (the fused learner-versus-greedy fragments)"
        assert not per_frame, 'per_frame belongs to frame_skip = K, learner = ...'
        return None
    assert isinstance(frame_skip, (int, np.integer)) and not isinstance(frame_skip, bool) and frame_skip >= 1, \
        f'frame_skip = {frame_skip!r}: a positive number of frames (examples/utils/wrappers.py FrameSkip)'
    assert learner in ('camera', 'target'), f"frame_skip needs learner = 'camera' or 'target' (got {learner!r}): the other team is the greedy agents"
    cameras = config.get('camera', {})
    assert learner != 'camera' or len(cameras.get('location', [])) + len(cameras.get('location_random_range', [])) > 0, \
        "learner = 'camera' needs cameras"
    for name, value in (('enhanced_observation', enhanced_observation), ('shared_field_of_view', shared_field_of_view)):
        assert value in (None, False, 'none'), f'{name} is not available with frame_skip: the fused launch packs plain rows'
    assert not camera_selection, 'camera_selection steps one frame per call: it does not combine with frame_skip'
    assert per_frame or learner != 'camera' or target_agent == 'greedy', \
        f"target_agent = {target_agent!r} is not available with frame_skip, learner = 'camera': the fused K-frame launch holds the Greedy agents (step per frame instead)"
    assert per_frame or learner != 'target' or camera_agent == 'greedy', \
        f"camera_agent = {camera_agent!r} is not available with frame_skip, learner = 'target': the fused K-frame launch holds the Greedy agents (step per frame instead)"
    other = target_reward_shaping if learner == 'camera' else camera_reward_shaping
    assert other is None, f"frame_skip with learner = {learner!r} shapes the learner's rewards only (the other team is the greedy agents)"
    shaping = camera_reward_shaping if learner == 'camera' else target_reward_shaping
    if shaping is not None:
        shaping = (dict(shaping[0]), shaping[1])
        (reward_coefficient_table if per_frame else fragment_coefficient_table)(learner, *shaping)
    spec = {'frame_skip': int(frame_skip), 'learner': learner, 'shaping': shaping}
    if per_frame:
        spec['per_frame'] = True
    return spec


class BatchedMultiAgentTracking(_ScenarioMixin):
    """N independent environments stepped by one kernel launch; every array is a torch tensor on the GPU.

        env = BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=4096)
        cam_obs, tgt_obs = env.reset()
        (cam_obs, tgt_obs), (r_cam, r_tgt), done, info = env.step((cam_act, tgt_act))

    `first_env_index` makes the RNG streams of a shard equal to those of the same environments in a
    larger single-GPU batch (sharding invariance).

    `camera_reward_shaping` / `target_reward_shaping` = (coefficients, reduction): the reference's AuxiliaryCameraRewards /
    AuxiliaryTargetRewards wrappers as one device launch behind every stepping call; `shaped_rewards()`
    returns the two tensors ([num_envs, agents], `reward_dtype`).  What step() and the rest return does not change.

    `frame_skip` = K with `learner` = 'camera' | 'target': the tail of the example trainers' chain -- MultiCamera | MultiTarget against
    the greedy opponents -> RelativeCoordinates -> RescaledObservation -> RepeatedRewardIndividualDone -> Auxiliary*Rewards ->
    FrameSkip(K) -- on the fused K-frame launch with the fragment launch behind it.  `relative_coordinates` /
    `rescaled_observation` then go to the fragment launch's column table instead of the packer (the fused launch packs plain rows),
    the learner's `*_reward_shaping` to its coefficients (the four terms that need every frame's state are refused).  reset() returns the
    learner's transformed rows [num_envs, agents, D]; step_fragment(joint_action) returns (obs, rewards [num_envs, agents], done
    [num_envs], info).  The row a restarted environment shows: by default a fused launch restarts finished episodes behind the launch
    without packing their first observation into caller buffers, so a restarted environment hands the learner its TERMINAL row with done
    set for one fragment -- as FrameSkip does before the trainer calls reset() -- and its next action is chosen on that row.  With
    `first_rows` = True (Engine.enable_fragment_rows(first_rows=True, final_obs=True)) the returned row of an environment the call
    restarted is instead the new episode's FIRST row, through the same transform -- the row env.reset() hands the reference's trainers --
    and `info` additionally holds 'restarted' [num_envs] bool and 'final_observation' [num_envs, agents, D], whose rows hold, for the
    restarted environments only, what the returned row would have been without it (the terminal row); rewards, done and the other
    info keys do not change.  Without `frame_skip` nothing about the class changes.

    `episode_records` = 'camera' | 'target' | True (the `learner` of a fragment environment, else 'target'): per-episode metric records
    for that team -- the reference's CustomMetricCallback keys -- kept on the device behind every stepping call (DESIGN.md section 3.12,
    Engine.enable_episode_records; attached behind the first reset()); `episodes()` returns the ones that arrived since its last call.  A learner step
    of a record is a frame, also under `frame_skip`.

    `training_information` = True: what the reference's mate.MoreTrainingInformation wrapper adds to the agents' infos, kept on the device
    behind every stepping call (Engine.enable_info_rows; attached behind the first reset()): `infos()` names the
    columns, `target_dones()` is the per-target done of RepeatedRewardIndividualDone(target_done_at_destination=True).

    `single_agent` = 'camera' | 'target': the reference's SingleCamera / SingleTarget -- the learner plays ONE agent of that team, the seat (`seat`:
    'auto' = slot n - 1, or drawn per episode under shuffle_entities; 'draw'; an index; an [num_envs] int32 tensor), its teammates are the on-device
    Greedy agents, `target_agent` / `camera_agent` / the mixtures name the OPPOSING team (Engine.enable_seat).  reset()
    returns the seat's rows [num_envs, D]; step_single(action) returns (seat_obs, reward, done, info) with info['seat'].

    `camera_messages` / `target_messages` = M: the environment's own send_messages / receive_messages for that team's LEARNER agents, as tensors -- M
    numbers of the observation dtype per message, routed on the device under the team's channel (no_communication / message_dropout /
    communication_range apply to them as to the scripted agents' exchange), with the reference's communication-edge counts alongside
    (send_messages, receive_messages, message_edges)."""

    def __init__(self, config=None, num_envs=1, device=0, seed=0, first_env_index=0, obs_dtype=torch.float32, auto_reset=True,
                 relative_coordinates=False, rescaled_observation=False, enhanced_observation=None, shared_field_of_view=None,
                 discrete_camera_levels=None, discrete_target_levels=None, state_rows=False,
                 camera_reward_shaping=None, target_reward_shaping=None, reward_dtype=torch.float64, camera_selection=None, frame_skip=None,
                 learner=None, first_rows=False, target_agent='greedy', camera_agent='greedy', episode_records=None, training_information=False,
                 target_mixture=None, camera_mixture=None, no_communication='none', message_dropout=0.0, communication_range=None, single_agent=None, seat='auto',
                 camera_messages=None, target_messages=None, per_frame=False, render_communication=None, **kwargs):
        assert state_rows in (False, True, 'normalized'), f"state_rows = {state_rows!r}: False, True or 'normalized'"
        self._setup_scenario(config, kwargs)
        self._policies_on = False                         # (enable_greedy_policies)
        self._target_shapers = {}                         # (auxiliary_target_rewards: one shaper per (coefficients, reduction))
        self._fragment_live = None                        # (_fragment_reset: the scalar record that says which environments were reset)
        self._fragment = fragment_arguments(self.config, frame_skip, learner, camera_reward_shaping, target_reward_shaping, enhanced_observation,
                                            shared_field_of_view, camera_selection, target_agent, camera_agent, per_frame=bool(per_frame))
        per_frame = bool(self._fragment and self._fragment.get('per_frame'))
        assert not per_frame or int(auto_reset) >= 1, 'per_frame: finished environments restart behind their fragment (auto_reset >= 1, counted in fragments)'
        assert target_agent == 'greedy' or not any(team in ('both', 'target') for team in (enhanced_observation, shared_field_of_view)), \
            f"target_agent = {target_agent!r} senses the cameras of its plain rows: no enhanced_observation / shared_field_of_view for the target team"
        assert camera_agent == 'greedy' or not any(team in ('both', 'camera') for team in (enhanced_observation, shared_field_of_view)), \
            f"camera_agent = {camera_agent!r} senses the targets of its plain rows: no enhanced_observation / shared_field_of_view for the camera team"
        assert camera_agent == 'greedy' or not camera_selection, f"camera_agent = {camera_agent!r}: camera_selection plays the camera team itself"
        self.target_agent, self.camera_agent = target_agent, camera_agent
        # target_mixture / camera_mixture: a name of SCRIPTED_AGENTS or a dict name -> weight -- the per-episode opponent mixture of that team
        # (Engine.set_opponent_mixture), checked now, installed by enable_greedy_policies
        self._mixtures = {team: spec for team, spec in (('target', target_mixture), ('camera', camera_mixture)) if spec is not None}
        for team, spec in self._mixtures.items():
            kinds, weights = mixture_table(spec)
            only_greedy = [SCRIPTED_AGENTS[k] for k, w in zip(kinds, weights) if w > 0.0] == ['greedy']
            assert not self._fragment or per_frame or self._fragment['learner'] == team or only_greedy, \
                f"{team}_mixture = {spec!r} is not available with frame_skip against that team: the fused K-frame launch holds the Greedy agents (step per frame instead)"
            assert team != 'camera' or not camera_selection, 'camera_mixture: camera_selection plays the camera team itself'
            assert (target_agent if team == 'target' else camera_agent) == 'greedy', f'{team}_mixture replaces {team}_agent: name the agent as a candidate'
        # no_communication / message_dropout / communication_range: the reference's NoCommunication, RandomMessageDropout and RestrictedCommunicationRange
        # wrappers as the channel of the teams the engine plays (Engine.set_channel), checked now, set by enable_greedy_policies
        self._channels = channel_table(no_communication, message_dropout, communication_range)
        for team, spec in zip(('camera', 'target'), self._channels):
            assert spec is None or not self._fragment or per_frame or self._fragment['learner'] == team, \
                f"a communication channel of the {team} team is not available with frame_skip against that team: the fused K-frame launch delivers every message (step per frame instead)"
            assert spec is None or team != 'camera' or (camera_agent == 'greedy' and 'heuristic' not in _names_of(camera_mixture)), \
                "a communication channel of the camera team needs Greedy cameras: HeuristicCameraAgent's fallback for a lost response is not on the device"
        assert episode_records in (None, True, 'camera', 'target'), f"episode_records = {episode_records!r}: None, True, 'camera' or 'target'"
        if episode_records is True:
            episode_records = self._fragment['learner'] if self._fragment else 'target'
        self._episode_team = episode_records              # (attached behind the first reset(): Engine.enable_episode_records)
        self._training_information = bool(training_information)      # (attached behind the first reset(): Engine.enable_info_rows)
        # single_agent = 'camera' | 'target': the reference's SingleCamera / SingleTarget (mate/wrappers/single_team.py) -- the learner plays ONE agent of that team,
        # the seat; its teammates are the on-device Greedy agents, target_agent / camera_agent / the mixtures keep their meaning for the OPPOSING team
        # (Engine.enable_seat).  Checked now, enabled with the policies.
        assert single_agent in (None, 'camera', 'target'), f"single_agent = {single_agent!r}: None, 'camera' or 'target'"
        if single_agent is None:
            assert isinstance(seat, str) and seat == 'auto', "seat = ... belongs to single_agent = 'camera' | 'target'"
        else:
            seat_mode_of(seat, bool(self.config['shuffle_entities']))
            assert not self._fragment, 'single_agent steps one frame per call: there is no fused K-frame seat flow (hold the action over K step_single calls)'
            assert not camera_selection, 'single_agent: camera_selection plays the camera team itself'
            assert (camera_agent if single_agent == 'camera' else target_agent) == 'greedy', \
                f"single_agent = {single_agent!r}: the seat's teammates are the Greedy agents ({single_agent}_agent names an opposing team's agent only)"
            assert set(_names_of(self._mixtures.get(single_agent))) <= {'greedy'}, f"single_agent = {single_agent!r}: the seat's teammates are the Greedy agents, not a mixture"
            assert not any(self._channels), "single_agent: the seat flow carries no communication channel (its agents' launch is not the channel launch)"
        self.single_agent, self._seat = single_agent, seat
        # camera_messages / target_messages = M: the environment's own send_messages / receive_messages for that team's learner agents, M numbers of the
        # observation dtype per message, routed on the device under the team's channel (Engine.enable_messages).  Checked now,
        # enabled behind the engine's construction.
        for name, width in (('camera_messages', camera_messages), ('target_messages', target_messages)):
            if width is not None and (isinstance(width, bool) or not isinstance(width, (int, np.integer)) or width < 1):
                raise ValueError(f'{name} = {width!r}: None or the message width, an integer >= 1')
        self._message_widths = (camera_messages, target_messages)
        self._info_frames = 0                             # frames of the last stepping call (target_dones: individual_done is NaN behind a multi-frame one)
        assert not first_rows or self._fragment, 'first_rows belongs to frame_skip = K, learner = ... (the per-step flows hand the first rows over already)'
        if self._fragment:      # the transforms and the shaping belong to the fragment launch (attached behind the first reset())
            self._fragment.update(relative_coordinates=bool(relative_coordinates), rescaled_observation=bool(rescaled_observation), dtype=reward_dtype,
                                  first_rows=bool(first_rows))
            if not per_frame:      # (per_frame: the packer transforms the rows, of reset() too)
                relative_coordinates = rescaled_observation = False
            camera_reward_shaping = target_reward_shaping = None
        self.num_envs, self.auto_reset = int(num_envs), int(auto_reset)   # 0 / False: never; 1 / True: immediately; k > 1: batched, every k-th call
        self.engine = Engine(self.config, self.num_envs, device=device, seed=seed, first_env_index=first_env_index, obs_dtype=obs_dtype)
        self.engine.keep_masks()      # (render() reads the engine's own mask words, which the stepping calls fill whether they bring their masks output or not)
        self.num_cameras, self.num_targets, self.num_obstacles = self.engine.num_cameras, self.engine.num_targets, self.engine.num_obstacles
        assert self._episode_team != 'camera' or self.num_cameras > 0, "episode_records = 'camera' needs cameras"
        self._setup_spaces()
        self.device = self.engine.device
        if relative_coordinates or rescaled_observation:   # the reference's RelativeCoordinates / RescaledObservation wrappers, fused
            self.engine.set_obs_transform(relative_coordinates, rescaled_observation)
        # EnhancedObservation(team=...) / SharedFieldOfView(team=...) of the reference: 'both', 'camera', 'target' or None
        modes = {'camera': 'plain', 'target': 'plain'}
        for name, team in (('shared', shared_field_of_view), ('enhanced', enhanced_observation)):
            if team in (None, False, 'none'):
                continue
            assert team in ('both', 'camera', 'target'), f'Invalid argument team {team!r}. Expect one of ("both", "camera", "target", "none").'
            for side in (('camera', 'target') if team == 'both' else (team,)):
                modes[side] = name
        if modes['camera'] != 'plain' or modes['target'] != 'plain':
            self.engine.set_obs_mode(**modes)
        # DiscreteCamera(levels) / DiscreteTarget(levels): integer action tensors are grid indices
        if discrete_camera_levels or discrete_target_levels:
            self.engine.set_action_grids(discrete_camera_levels, discrete_target_levels)
        for team, width in enumerate(self._message_widths):
            if width is not None:
                assert (self.num_cameras, self.num_targets)[team] > 0, f"{('camera', 'target')[team]}_messages: the scenario has no such agents"
                self.engine.enable_messages(team, int(width), pairwise=True, addressed=True)

        # the global state for centralised critics (RLlibMultiAgentCentralizedTraining, examples/utils/wrappers.py:114-121, 170-225):
        # True = raw rows, 'normalized' = mate.normalize_observation(state, state_space) fused into the row writer
        self.state_rows = state_rows
        if state_rows == 'normalized':
            self.state_space = consts.normalized_state_space_of(self.num_cameras, self.num_targets, self.num_obstacles)
        # AuxiliaryCameraRewards / AuxiliaryTargetRewards (the last wrapper of the example trainers' chains) as a launch attached to the
        # engine: (coefficients, reduction) per team, checked now, attached behind the first reset() (Engine.enable_reward_rows)
        self._reward_shaping = {team: (dict(spec[0]), spec[1]) for team, spec in (('camera', camera_reward_shaping), ('target', target_reward_shaping))
                                if spec is not None}
        for team, spec in self._reward_shaping.items():
            reward_coefficient_table(team, *spec)
        self._reward_dtype = reward_dtype
        # HierarchicalCamera(MultiCamera(env, GreedyTargetAgent()), multi_selection) of the reference's hierarchical camera trainers
        # (examples/hrl/wrappers.py), one frame per call: 'multi' / 'single'; attached behind the first reset() (Engine.enable_selection)
        assert camera_selection in (None, 'multi', 'single'), f"camera_selection = {camera_selection!r}: None, 'multi' or 'single'"
        self.camera_selection = camera_selection
        # render_communication = duration: mate.RenderCommunication(env, duration) -- the per-pair countdowns on the device behind every per-step call, the
        # dashed arrows in render() (Engine.enable_communication_trace)
        if render_communication is not None and (isinstance(render_communication, bool) or not 1 <= int(render_communication) <= 255):
            raise ValueError(f'render_communication = {render_communication!r}: None or the duration, an integer in [1, 255]')
        assert render_communication is None or not single_agent, 'render_communication: the seat flow carries no communication channel, so its teammates draw no arrows'
        assert render_communication is None or not self._fragment or per_frame, 'render_communication steps one frame per call: the fused K-frame launch keeps no per-frame edges (per_frame=True instead)'
        self._render_communication = None if render_communication is None else int(render_communication)
        if camera_selection:
            assert self.num_cameras > 0, 'camera_selection needs cameras'
            self.enable_greedy_policies()
        if self._fragment or ((target_agent != 'greedy' or camera_agent != 'greedy') and not camera_selection) or ((self._mixtures or any(self._channels) or single_agent) and not self._policies_on):
            self.enable_greedy_policies()
        self._enable_render_communication()

    def _enable_render_communication(self):
        if self._render_communication:
            teams = [team for team, n in (('camera', self.num_cameras), ('target', self.num_targets)) if n > 0]
            self.engine.enable_communication_trace(teams=teams, duration=self._render_communication)

    def communication_trace(self):
        """(camera remaining, target remaining): uint8 [num_envs, n, n] views of the engine's matrices, [sender][recipient] -- RenderCommunication's
        camera_comm_matrix / target_comm_matrix per environment (None for a team without agents).  Built with render_communication = duration."""
        assert self._render_communication, 'built without render_communication = duration'
        return tuple(self.engine.communication_trace(team) if n > 0 else None for team, n in enumerate((self.num_cameras, self.num_targets)))

    def seed(self, seed):
        self.engine.seed(int(seed))
        return [int(seed)]

    def state(self):
        """The global state of every environment, [num_envs, state_dim] on the GPU (state() of the reference, environment.py:894-906,
        per environment; normalised when built with state_rows='normalized').  With `state_rows` the engine keeps the tensor current
        behind every reset / step / rollout and this returns it (the same tensor every time); without, one on-demand launch."""
        if self.state_rows and self.engine.state is not None:
            return self.engine.state
        return self.engine.state_rows(normalize=self.state_rows == 'normalized')

    def shaped_rewards(self):
        """(camera rows [num_envs, num_cameras], target rows [num_envs, num_targets]) of the step that last ran -- the shaped rewards of
        `camera_reward_shaping` / `target_reward_shaping` (None for a team without one), written on the device behind every stepping
        call and ahead of the auto-reset: the terminal step's rewards too.  The same tensors every time, from the first reset() on."""
        return self.engine.camera_reward_rows, self.engine.target_reward_rows

    def reset(self, env_mask=None):
        out = self.engine.reset(env_mask)
        if self.state_rows and self.engine.state is None:      # (rows attach to records that exist: from the first reset on)
            self.engine.enable_state_rows(normalize=self.state_rows == 'normalized')
        if self._reward_shaping and self.engine.reward_coefficients is None:
            self.engine.enable_reward_rows(camera=self._reward_shaping.get('camera'), target=self._reward_shaping.get('target'), dtype=self._reward_dtype)
        if self.camera_selection and self.engine.selection is None:
            self.engine.enable_selection(self.camera_selection == 'multi')
        if self._training_information and not self.engine._info_attached():      # (behind the reward rows)
            self.engine.enable_info_rows()
        for shaper in self._target_shapers.values():
            shaper.observe_reset()
        if self._fragment:
            out = self._fragment_reset(env_mask)
        if self.single_agent:
            out = self.engine.seat_rows()[0]
        if self._episode_team and self.engine.episode_team is None:      # (behind the reward rows, which its launch reads)
            self.engine.enable_episode_records(self._episode_team)
        return out

    def render(self, envs=(0,), size=800, headings=None):
        """uint8 [k, size, size, 3] on the device: the reference's render(mode='rgb_array') pictures of the environments `envs` (Engine.render; DESIGN.md
        section 3.20).  `headings`: [k, num_targets] degrees, the render-only target_orientations the engine does not keep (None: zeros)."""
        return self.engine.render(list(envs), size=size, headings=headings)

    def _want_masks(self):
        """The calls that may go without the view masks bring them for the reward launch, for the camera team's num_tracked record and for the
        training-information rows."""
        return bool(self._reward_shaping) or self._episode_team == 'camera' or self._training_information

    def infos(self):
        """The training information of the step that last ran (`training_information`): {name: view} of Engine.info() -- num_tracked,
        is_sensed [num_envs, num_cameras]; goal, goal_distance, individual_done, is_tracked, is_colliding [num_envs, num_targets];
        warehouse_distances [num_envs, num_targets, 4]; remaining_cargo_counts, awaiting_cargo_counts [num_envs, 4]; remaining_cargoes
        [num_envs, 4, 4], all f64 -- plus the common scalar columns of that step by name (coverage_rate, real_coverage_rate,
        mean_transport_rate, num_delivered_cargoes, normalized_raw_reward).  Written ahead of the auto-reset: the terminal step's values too.
        Behind a multi-frame call (rollout_*, step_fragment) the rows describe its last frame and individual_done is NaN."""
        assert self._training_information, 'built without training_information=True'
        assert self.engine._info_attached(), 'reset() first'
        out = self.engine.info()
        out.update(self._columns(self._info_scalars())[2])
        return out

    def _info_scalars(self):
        """The scalar records [num_envs, 8] of the frame the training-information rows describe: the last frame of the last stepping call."""
        rollout = self.engine._rollout
        if self._info_frames > 1 and rollout is not None:
            return rollout['scalars'][self._info_frames - 1]
        return self.engine.scalars

    def target_dones(self):
        """[num_envs, num_targets] bool: the targets that delivered their cargo at the step that last ran -- the `done` of the reference's
        RepeatedRewardIndividualDone(target_done_at_destination=True).  Raises behind a multi-frame call, where the column is NaN."""
        assert self._training_information, 'built without training_information=True'
        assert self.engine._info_attached(), 'reset() first'
        if self._info_frames > 1:
            raise RuntimeError(f'target_dones() behind a call of {self._info_frames} frames: a delivery between the frames cannot be seen from its end state '
                               '(individual_done is NaN); step frame by frame for per-target dones')
        return self.engine.info_target_rows[:, :, 6] > 0

    def episodes(self):
        """The episode records that arrived since the last call (`episode_records`): {column: [M] f64 tensor} for Engine.EPISODE_COLUMNS,
        oldest first, and 'dropped': how many more the ring lost before they were read.  Waits for the stream's launches."""
        assert self._episode_team, "built without episode_records = 'camera' | 'target' | True"
        assert self.engine.episode_team is not None, 'reset() first'
        records, dropped = self.engine.episode_records()
        out = {name: records[:, k] for k, name in enumerate(self.engine.EPISODE_COLUMNS)}
        out['dropped'] = dropped
        return out

    def _fragment_reset(self, env_mask=None):
        """The learner's transformed rows of the observation reset() has just packed: the fragment launch on demand, one frame.  A masked
        reset repacks the listed environments only: the others' one-frame record says done = 2, so their fragment rows stay as they are."""
        spec, eng = self._fragment, self.engine
        transform = {'relative_coordinates': spec['relative_coordinates'], 'rescaled_observation': spec['rescaled_observation']}
        if eng.fragment_team is None:
            eng.enable_fragment_rows(spec['learner'], spec['frame_skip'], shaping=spec['shaping'], dtype=spec['dtype'], first_rows=spec['first_rows'],
                                     final_obs=spec['first_rows'], per_frame=bool(spec.get('per_frame')), **transform)
        rows = eng.camera_obs if spec['learner'] == 'camera' else eng.target_obs
        if self._fragment_live is None:      # (a scalar record that says "this frame ran": the step's own may be older than the reset)
            self._fragment_live = torch.zeros((self.num_envs, 8), dtype=torch.float32, device=self.device)
        if env_mask is None:
            self._fragment_live[:, 2] = 0.0
        else:
            self._fragment_live[:, 2] = torch.where(env_mask.to(device=self.device).bool().reshape(-1), 0.0, 2.0)
        if spec.get('per_frame'):      # (the packer has transformed the rows: the frame launch's last phase copies the live ones)
            eng.frame_fragment(spec['learner'], rows, self._fragment_live, spec['frame_skip'] - 1, spec['frame_skip'], out={'obs': eng.fragment_obs})
        else:
            eng.fragment_rows(spec['learner'], rows, self._fragment_live, out={'obs': eng.fragment_obs}, **transform)
        return eng.fragment_obs

    def step_fragment(self, joint_action):
        """One fragment: `joint_action` ([num_envs, agents, 2] or grid indices) held for frame_skip frames against the greedy opponents in
        one launch, reduced by the fragment launch.  Returns (obs [num_envs, agents, D], rewards [num_envs, agents], done [num_envs],
        info): `rewards` is the shaped sum with `*_reward_shaping`, else the learner's team reward repeated per agent
        (RepeatedRewardIndividualDone); `info` holds FrameSkip's reduced keys ('sum': the raw and normalised rewards; 'mean': the two
        coverage rates; 'last': mean_transport_rate, num_delivered_cargoes) and 'frames' [num_envs], the frames that ran; built with
        first_rows=True also 'restarted' [num_envs] bool and 'final_observation' [num_envs, agents, D].  The tensors are
        the engine's own, rewritten by the next call.  See the class docstring for the row a restarted environment shows."""
        assert self._fragment, 'built without frame_skip = K, learner = ...'
        spec, eng = self._fragment, self.engine
        assert eng.fragment_team is not None, 'reset() first'
        if spec.get('per_frame'):      # K per-step calls, each folded in by the frame launch; the restart interval counts engine calls
            self._info_frames = 1
            eng.step_fragment_frames(spec['learner'], joint_action, auto_reset=int(self.auto_reset) * spec['frame_skip'])
        else:
            self._info_frames = spec['frame_skip']
            eng.rollout_versus_greedy(spec['learner'], joint_action, spec['frame_skip'], auto_reset=int(self.auto_reset), want_masks=self._training_information)
        camera = spec['learner'] == 'camera'
        sums, means = eng.fragment_rewards, eng.fragment_info
        if eng.fragment_shaped is not None:
            rewards = eng.fragment_shaped
        else:
            rewards = sums[:, 0 if camera else 1, None].expand(-1, eng.fragment_obs.shape[1])
        info = {'raw_reward': sums[:, 0 if camera else 1], 'normalized_raw_reward': sums[:, 3 if camera else 2],
                'coverage_rate': means[:, 0], 'real_coverage_rate': means[:, 1], 'mean_transport_rate': means[:, 2],
                'num_delivered_cargoes': means[:, 3], 'frames': eng.fragment_frames}
        if spec['first_rows']:
            info.update(restarted=eng.fragment_restarted, final_observation=eng.fragment_final_obs)
        return eng.fragment_obs, rewards, eng.fragment_done > 0, info

    @staticmethod
    def _columns(s):
        """(rewards, done column, info) of scalar records [..., 8], by SCALAR_NAMES."""
        col = dict(zip(SCALAR_NAMES, s.unbind(-1)))
        info = {key: col[key] for key in ('coverage_rate', 'real_coverage_rate', 'mean_transport_rate', 'num_delivered_cargoes')}
        info['normalized_raw_reward'] = col['normalized_target_team_reward']
        return (col['camera_team_reward'], col['target_team_reward']), col['done'], info

    def _result(self):
        self._info_frames = 1
        rewards, done, info = self._columns(self.engine.scalars)
        return (self.engine.camera_obs, self.engine.target_obs), rewards, done > 0, info

    def step(self, action):
        cam_act, tgt_act = action
        self.engine.step(cam_act, tgt_act, auto_reset=self.auto_reset)
        return self._result()

    def step_random(self):
        """One step under the on-device uniform random policy (no action tensors)."""
        self.engine.step_random(auto_reset=self.auto_reset, want_masks=self._want_masks())
        return self._result()

    def _rollout_result(self, out):
        cam, tgt, s = out
        self._info_frames = int(s.shape[0])
        rewards, done, info = self._columns(s)
        info['skipped'] = done == 2          # slots after the end of an episode inside the launch (no step, stale rows)
        return (cam, tgt), rewards, done == 1, info

    def rollout_random(self, steps):
        """`steps` env.step(random action) iterations in ONE launch (the fastest flow, profiles/HISTORY.md 3.1b): every tensor of
        step()'s result with a leading [steps] axis.  Finished episodes restart after the launch."""
        return self._rollout_result(self.engine.rollout_random(steps, auto_reset=int(self.auto_reset), want_masks=self._want_masks()))

    def rollout_greedy(self, steps):
        """`steps` iterations of mate.group_step with the reference's Greedy camera / target agents + env.step in ONE
        launch (agents on the device, profiles/HISTORY.md 3.1c)."""
        self._need_policies()
        return self._rollout_result(self.engine.rollout_greedy(steps, auto_reset=int(self.auto_reset), want_masks=self._want_masks()))

    def enable_greedy_policies(self):
        self.engine.enable_policies(target_agent=self.target_agent, camera_agent=self.camera_agent)
        for team, spec in self._mixtures.items():
            if self.engine.mixtures[0 if team == 'camera' else 1] is None:
                self.engine.set_opponent_mixture(team, spec)
        for team, spec in enumerate(self._channels):
            if spec is not None and self.engine.channels[team] is None:
                self.engine.set_channel(team, **spec)
        if self.single_agent and self.engine.seat_obs is None:
            assert (self.num_cameras if self.single_agent == 'camera' else self.num_targets) > 0, f'single_agent = {self.single_agent!r}: the scenario has no such agents'
            self.engine.enable_seat(self.single_agent, self._seat)
        self._policies_on = True
        if getattr(self, '_render_communication', None) and self.engine.trace_duration:      # (enabled behind the construction: the engine-played teams' transparent channels)
            self._enable_render_communication()

    def communication_edges(self):
        """((camera sent, camera delivered), (target sent, target delivered)): [num_envs, n, n] int8 tensors on the GPU, [sender][recipient], as the
        last agents' launch with a channel left them -- what the on-device agents handed to their channel and what arrived (the reference's
        camera_communication_edges / target_communication_edges, per environment).  Views of engine-owned memory: copy what must outlive the next step."""
        self._need_policies()
        return tuple(self.engine.channel_edges(team) for team in (0, 1))

    def send_messages(self, team, payload, address=None, round=0):
        """The environment's send_messages for the learner agents of `team` ('camera' / 'target'; built with camera_messages / target_messages = M), one
        call for the whole team and batch: `payload` is [num_envs, n, M] (one content per sender, to everyone it addresses) or [num_envs, n, n, M]
        ([sender][recipient]); `address` [num_envs, n, n], non-zero = send, None: every sender broadcasts to every slot of its team, its own included
        (route_messages).  At most one message per ordered pair and call; `round` (0..15) tells the calls between two steps apart.  The messages pass the
        team's channel (no_communication / message_dropout / communication_range) at once; receive_messages(team) reads what arrived."""
        code = 0 if team in ('camera', 0) else 1
        assert team in ('camera', 'target', 0, 1) and self._message_widths[code] is not None, f'built without {team}_messages = M'
        eng = self.engine
        n, M = (self.num_cameras, self.num_targets)[code], int(self._message_widths[code])
        payload = torch.as_tensor(payload, device=self.device).to(eng.obs_dtype)
        assert tuple(payload.shape) in ((self.num_envs, n, M), (self.num_envs, n, n, M)), f'payload: [num_envs, n, M] or [num_envs, n, n, M], got {tuple(payload.shape)}'
        eng.message_payload[code].copy_(payload if payload.dim() == 4 else payload[:, :, None, :].expand(-1, -1, n, -1))
        if address is None:
            eng.message_address[code].fill_(1)
        else:
            address = torch.as_tensor(address, device=self.device)
            assert tuple(address.shape) == (self.num_envs, n, n), f'address: [num_envs, n, n], got {tuple(address.shape)}'
            eng.message_address[code].copy_(address != 0)
        eng.route_messages(code, round)

    def receive_messages(self, team):
        """(inbox, delivered) of the last send_messages(team): inbox [num_envs, n recipient, n sender, M], the delivered contents, zeros where nothing was
        sent or arrived -- agent r's messages are inbox[:, r], in sender order; delivered [num_envs, n, n] int8, [sender][recipient].  The engine's own
        tensors, rewritten by the next send_messages(team)."""
        code = 0 if team in ('camera', 0) else 1
        assert team in ('camera', 'target', 0, 1) and self._message_widths[code] is not None, f'built without {team}_messages = M'
        return self.engine.message_inbox[code], self.engine.message_edges(code)['delivered']

    def message_edges(self, team):
        """{'sent', 'delivered', 'step_edges', 'total_edges', 'agent_edges'} of the team's learner messages (Engine.message_edges): 'step_edges' is the
        reference's *_communication_edges (the deliveries since the last step), 'total_edges' its *_total_communication_edges as the last step left them,
        'agent_edges'[:, a] = (out_communication_edges, in_communication_edges) of agent a's `info`."""
        return self.engine.message_edges(team)

    def step_single(self, action, **replay):
        """One step of SingleCamera / SingleTarget (`single_agent`): `action` is the seat's, [num_envs, 2] reals or [num_envs] grid indices; the teammates
        and the opponents act on the device.  Returns (seat_obs [num_envs, D], reward [num_envs], done [num_envs], info): the seat's row of the new
        observations -- of the NEW episode's seat where the call restarted the environment --, the team's reward and done, and step()'s info plus
        'seat' [num_envs] int32, the seat that row belongs to, and 'seat_acted', the seat whose action the step consumed.  The tensors are the engine's
        own, rewritten by the next call.  `replay`: recorded draws, as Engine.step_seated takes them."""
        assert self.single_agent, "built without single_agent = 'camera' | 'target'"
        self.engine.step_seated(action, auto_reset=self.auto_reset, **replay)
        _, rewards, done, info = self._result()
        info.update(seat=self.engine.seat_index, seat_acted=self.engine.seat_acted)
        return self.engine.seat_obs, rewards[0 if self.single_agent == 'camera' else 1], done, info

    def step_versus_greedy(self, team, joint_action):
        """MultiCamera(env, target_agent=GreedyTargetAgent()) for team = 'camera', MultiTarget(env,
        camera_agent=GreedyCameraAgent()) for team = 'target' (mate/wrappers/single_team.py:281-306): the caller acts for
        `team`, the greedy agents of the other team act on the device.  step()'s full result (both teams' observations
        and rewards; a single-team learner reads its own half)."""
        self._need_policies()
        self.engine.step_versus_greedy(team, joint_action, auto_reset=self.auto_reset)
        return self._result()

    def rollout_versus_greedy(self, team, joint_action, frame_skip):
        """FrameSkip(MultiCamera | MultiTarget, frame_skip) in one launch (examples/utils/wrappers.py:301-323): rollout-shaped
        result; `rewards.sum(0)` is the wrapper's reward, `done.any(0)` its done."""
        self._need_policies()
        return self._rollout_result(self.engine.rollout_versus_greedy(team, joint_action, frame_skip, auto_reset=int(self.auto_reset), want_masks=self._want_masks()))

    def step_selected(self, selection, **replay):
        """One frame of HierarchicalCamera.step (examples/hrl/wrappers.py:93-152) for every environment: `selection` is [num_envs,
        num_cameras, num_targets] of 0 / 1 (camera_selection='multi'; or the packed [num_envs, num_cameras] words) or [num_envs,
        num_cameras] indices in [0, num_targets] ('single'; num_targets = none), integers, checked for shape and dtype only.  The
        executor and the greedy targets act on the device.  Returns step()'s result; `selection_info()` and `action_mask()` follow it.
        The wrapper's frame_skip = K is K calls with the selection held, in an environment built with auto_reset = K: an environment
        that finishes inside the fragment idles for the rest of it (done stays set, selection_info()['frames'] is 0: add neither its
        rewards nor its metrics) and restarts behind the fragment's last call.  (In a graph: Engine.make_stepper(versus='selection',
        frame_skip=K).)  `replay`: recorded draws, as Engine.step_selected takes them (policy_tape, tape_ct, tape_goal)."""
        assert self.camera_selection, "built without camera_selection='multi' | 'single'"
        eng = self.engine
        assert eng.selection is not None, 'reset() first'
        eng.selection.copy_(eng.encode_selection(selection))
        eng.step_selected(auto_reset=self.auto_reset, **replay)
        return self._result()

    def selection_info(self):
        """The wrapper's infos of the frame step_selected last ran, {name: [num_envs, num_cameras] f64} for the four SELECTION_METRICS,
        and 'frames': [num_envs] int32 -- 1, or 0 for an environment that idles behind its terminal frame (its metrics are zero)."""
        eng = self.engine
        info = {name: eng.selection_metrics[:, :, k] for k, name in enumerate(eng.SELECTION_METRICS)}
        info['frames'] = eng.selection_frames
        return info

    def action_mask(self):
        """action_mask() (examples/hrl/wrappers.py:166-175) of the camera rows the learner sees next: [num_envs, num_cameras, 2 num_targets]
        ('multi': even entries 1) or [num_envs, num_cameras, num_targets + 1] ('single': last entry 1) u8, the same tensor every time."""
        return self.engine.action_mask

    def masks(self):
        return self.engine.unpack_masks()

    AUXILIARY_REWARD_KEYS = CAMERA_REWARD_KEYS

    def auxiliary_camera_rewards(self, coefficients, reduction='none'):
        """Per-camera shaped rewards of the last step, the reference's AuxiliaryCameraRewards wrapper
        (wrappers/auxiliary_camera_rewards.py:110-176) with constant coefficients: a weighted sum of the team reward,
        the coverage / transport metrics of the step record, the number of targets each camera tracks and a
        baseline; `reduction` in ('none', 'mean', 'sum', 'max', 'min') shares one value among the cameras.
        Returns a [num_envs, num_cameras] tensor on the GPU (a handful of elementwise ops on the [N, 8] step record
        and the packed masks: nothing here touches the observation bytes).  `soft_coverage_score` (:181-239) is one more
        small kernel over the outer occlusion boundary, which the engine builds from the first request on."""
        reward_coefficient_table('camera', coefficients, reduction)
        s = self.engine.scalars.double()
        N, Nc, Nt = self.num_envs, self.num_cameras, self.num_targets
        bits = torch.arange(Nc * Nt, device=self.device)
        words = self.engine.masks.long()[:, bits // 32]                       # camera_target_view_mask lives in the first words
        seen = ((words >> (bits % 32)) & 1).view(N, Nc, Nt)
        terms = {'raw_reward': s[:, 0:1].expand(N, Nc), 'coverage_rate': s[:, 3:4].expand(N, Nc),
                 'real_coverage_rate': s[:, 4:5].expand(N, Nc), 'mean_transport_rate': s[:, 5:6].expand(N, Nc),
                 'num_tracked': seen.sum(dim=2).double(), 'baseline': torch.ones((N, Nc), dtype=torch.float64, device=self.device)}
        if 'soft_coverage_score' in coefficients:
            self.engine.need_outer_boundary()
            terms['soft_coverage_score'] = self.engine.soft_coverage()[1]
        reward = torch.zeros((N, Nc), dtype=torch.float64, device=self.device)
        for key, coefficient in coefficients.items():
            reward = reward + float(coefficient) * terms[key]
        if reduction != 'none':
            shared = {'mean': reward.mean(dim=1), 'sum': reward.sum(dim=1), 'max': reward.max(dim=1).values, 'min': reward.min(dim=1).values}[reduction]
            reward = shared[:, None].expand(N, Nc)
        return reward

    def auxiliary_target_rewards(self, coefficients, reduction='none'):
        """Per-target shaped rewards of the last step, the reference's AuxiliaryTargetRewards wrapper
        (wrappers/auxiliary_target_rewards.py:118-216) with constant coefficients: [num_envs, num_targets] on the GPU.  Call
        it after every step (its `sparse_delivery` term compares the goals with those of the previous call; see
        mate_amd/auxiliary_rewards.py)."""
        key = (tuple(sorted(coefficients.items())), reduction)
        if key not in self._target_shapers:
            self._target_shapers[key] = AuxiliaryTargetRewards(self.engine, coefficients, reduction)
        return self._target_shapers[key]()

    def state_dict(self):
        return self.engine.state_dict()

    def close(self):
        self.engine.close()
