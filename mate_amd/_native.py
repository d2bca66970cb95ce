"""ctypes binding of ``mate_amd/lib/libmate_engine.so`` (C ABI: ``include/mate_engine.h``).

There is no CPU fallback: if the HIP library is missing or fails to load this
module raises, and every engine call that returns a non-zero status raises
``EngineError`` carrying ``mate_engine_last_error()``.
"""
import ctypes
import os

__all__ = ['lib', 'load', 'EngineError', 'MateConfig', 'MateLayout', 'MateStepIO', 'MatePolicyTape', 'MateRewardRows', 'MateFragmentRows', 'MateFirstRows', 'MateFrameFragments', 'LIB_PATH', 'check', 'EXPORTED_SYMBOLS']

LIB_PATH = os.environ.get('MATE_ENGINE_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'lib', 'libmate_engine.so')

class EngineError(RuntimeError):
    """A C-ABI call failed (status code + message from the engine)."""

    def __init__(self, code, message):
        super().__init__(f'mate_engine error {code}: {message}')
        self.code = code


class MateConfig(ctypes.Structure):
    _fields_ = [
        ('num_cameras', ctypes.c_int32), ('num_targets', ctypes.c_int32), ('num_obstacles', ctypes.c_int32),
        ('max_episode_steps', ctypes.c_int32), ('sparse_reward', ctypes.c_int32),
        ('num_cargoes_per_target', ctypes.c_int32), ('shuffle_entities', ctypes.c_int32),
        ('targets_start_with_cargoes', ctypes.c_int32),
        ('high_capacity_target_split', ctypes.c_double), ('bounty_factor', ctypes.c_double),
        ('transmittance', ctypes.c_double),
        ('camera_radius', ctypes.c_double), ('camera_min_viewing_angle', ctypes.c_double),
        ('camera_max_sight_range', ctypes.c_double), ('camera_rotation_step', ctypes.c_double),
        ('camera_zooming_step', ctypes.c_double),
        ('target_step_size', ctypes.c_double), ('target_sight_range', ctypes.c_double),
        ('obstacle_radius_range', ctypes.c_double * 2),
        ('camera_location_ranges', ctypes.POINTER(ctypes.c_double)),
        ('target_location_ranges', ctypes.POINTER(ctypes.c_double)),
        ('obstacle_location_ranges', ctypes.POINTER(ctypes.c_double)),
        ('obs_dtype', ctypes.c_int32),
    ]


class MateLayout(ctypes.Structure):
    _fields_ = [(name, ctypes.c_int32) for name in (
        'camera_obs_dim', 'target_obs_dim', 'state_dim', 'mask_words', 'bit_camera_target', 'bit_camera_camera',
        'bit_target_row', 'bit_camera_obstacle', 'export_width', 'lut_capacity', 'scalars_per_env', 'specialised')]


class MatePolicyTape(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in (
        'camera_resample_u_dev', 'camera_sample_u_dev', 'camera_delay_dev', 'target_choice_u_dev',
        'target_resample_u_dev', 'target_sample_u_dev', 'target_reset_sample_u_dev')]


class MateStepIO(ctypes.Structure):
    _fields_ = [
        ('camera_actions_dev', ctypes.c_void_p), ('target_actions_dev', ctypes.c_void_p), ('act_dtype', ctypes.c_int32),
        ('tape_camera_target_dev', ctypes.c_void_p), ('tape_goal_dev', ctypes.c_void_p),
        ('camera_obs_dev', ctypes.c_void_p), ('target_obs_dev', ctypes.c_void_p),
        ('scalars_dev', ctypes.c_void_p), ('masks_dev', ctypes.c_void_p),
    ]


class MateRewardRows(ctypes.Structure):
    """mate_reward_rows: the attachment of the shaped-reward launch (mate_engine_enable_reward_rows)."""
    _fields_ = [
        ('camera_rows_dev', ctypes.c_void_p), ('target_rows_dev', ctypes.c_void_p),
        ('camera_terms_dev', ctypes.c_void_p), ('target_terms_dev', ctypes.c_void_p),
        ('out_dtype', ctypes.c_int32), ('camera_reduction', ctypes.c_int32), ('target_reduction', ctypes.c_int32),
        ('accumulate', ctypes.c_int32), ('soft_coverage', ctypes.c_int32),
        ('camera_coefficients_dev', ctypes.c_void_p), ('target_coefficients_dev', ctypes.c_void_p),
    ]


class MateFragmentRows(ctypes.Structure):
    """mate_fragment_rows: the FrameSkip fragment launch (mate_engine_enable_fragment_rows / mate_engine_fragment_rows)."""
    _fields_ = [
        ('team', ctypes.c_int32), ('obs_dev', ctypes.c_void_p), ('rewards_dev', ctypes.c_void_p), ('info_dev', ctypes.c_void_p),
        ('done_dev', ctypes.c_void_p), ('frames_dev', ctypes.c_void_p), ('shaped_dev', ctypes.c_void_p),
        ('out_dtype', ctypes.c_int32), ('reduction', ctypes.c_int32), ('coefficients', ctypes.c_void_p),
        ('column_sub', ctypes.c_void_p), ('column_flag', ctypes.c_void_p), ('column_scale', ctypes.c_void_p), ('column_bias', ctypes.c_void_p),
    ]


class MateFirstRows(ctypes.Structure):
    """mate_first_rows: first rows of restarted episodes behind the attached fragment rows (mate_engine_enable_first_rows)."""
    _fields_ = [('rows_dev', ctypes.c_void_p), ('scalars_dev', ctypes.c_void_p), ('final_obs_dev', ctypes.c_void_p)]


class MateFrameFragments(ctypes.Structure):
    """mate_frame_fragments: the FrameSkip fragment built frame by frame behind the per-step calls (mate_engine_enable_frame_fragments / mate_engine_frame_fragment)."""
    _fields_ = [
        ('team', ctypes.c_int32), ('frames', ctypes.c_int32), ('obs_dev', ctypes.c_void_p), ('final_obs_dev', ctypes.c_void_p),
        ('restarted_dev', ctypes.c_void_p), ('rewards_dev', ctypes.c_void_p), ('info_dev', ctypes.c_void_p), ('done_dev', ctypes.c_void_p),
        ('frames_dev', ctypes.c_void_p), ('shaped_dev', ctypes.c_void_p), ('out_dtype', ctypes.c_int32), ('first_rows', ctypes.c_int32),
    ]


class MateChannel(ctypes.Structure):
    """mate_channel: one team's communication channel (mate_engine_set_channel)."""
    _fields_ = [('disabled', ctypes.c_int32), ('range_limit', ctypes.c_double), ('dropout_rate', ctypes.c_double), ('mask_dev', ctypes.c_void_p)]


class MateMessageRows(ctypes.Structure):
    """mate_message_rows: one team's message buffers (mate_engine_enable_messages)."""
    _fields_ = [('width', ctypes.c_int32), ('pairwise', ctypes.c_int32), ('payload_dev', ctypes.c_void_p), ('address_dev', ctypes.c_void_p), ('inbox_dev', ctypes.c_void_p)]


P, I32, I64, U64, INT = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int
F64P, IO, TAPE = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(MateStepIO), ctypes.POINTER(MatePolicyTape)

# The C ABI of include/mate_engine.h, once: name -> (restype, argtypes).  load() applies it; tests/test_host_logic.py holds every
# entry's arity and every structure's member names against the header.
PROTOTYPES = {
    'mate_engine_last_error': (ctypes.c_char_p, []),
    'mate_engine_abi_version': (INT, []),
    'mate_engine_create': (INT, [ctypes.POINTER(MateConfig), I64, I32, U64, U64, ctypes.POINTER(P)]),
    'mate_engine_destroy': (INT, [P]),
    'mate_engine_get_layout': (INT, [P, ctypes.POINTER(MateLayout)]),
    'mate_engine_seed': (INT, [P, U64]),
    'mate_engine_set_obs_transform': (INT, [P, I32, P, P, P, P]),
    'mate_engine_set_obs_mode': (INT, [P, I32, I32]),
    'mate_engine_set_action_grids': (INT, [P, P, I32, P, I32]),
    'mate_engine_reset': (INT, [P, P, IO, P]),
    'mate_engine_reset_tape': (INT, [P, P, IO, P, I32, P, P]),
    'mate_engine_step': (INT, [P, IO, I32, P]),
    'mate_engine_device_tick': (INT, [P, I32, P]),
    'mate_engine_set_episode_stats': (INT, [P, P]),
    'mate_engine_snapshot_episode_stats': (INT, [P, P, P]),
    'mate_engine_step_random': (INT, [P, IO, I32, P]),
    'mate_engine_rollout_random': (INT, [P, IO, I32, I32, P]),
    'mate_engine_policy_enable': (INT, [P]),
    'mate_engine_step_greedy': (INT, [P, IO, TAPE, I32, P]),
    'mate_engine_step_versus_greedy': (INT, [P, I32, IO, TAPE, I32, P]),
    'mate_engine_policy_actions': (INT, [P, P, P, P]),
    'mate_engine_policy_greedy_target_actions': (INT, [P, P, P]),
    'mate_engine_set_target_opponent': (INT, [P, I32]),
    'mate_engine_set_camera_opponent': (INT, [P, I32]),
    'mate_engine_heuristic_camera_tables': (INT, [P, P, P, P]),
    'mate_engine_heuristic_camera_tape': (INT, [P, P, P]),
    'mate_engine_heuristic_camera_goals': (INT, [P, P, P, P]),
    'mate_engine_set_opponent_mixture': (INT, [P, I32, ctypes.POINTER(I32), F64P, I32, I32]),
    'mate_engine_scripted_tape': (INT, [P, P, P, P, P, P, P, P, P]),
    'mate_engine_scripted_memory': (INT, [P, I32, P, P, P, P, P, P, P]),
    'mate_engine_scripted_external': (INT, [P, I32, ctypes.POINTER(P)]),
    'mate_engine_scripted_rows': (INT, [P, I32, I32, P, P]),
    'mate_engine_set_channel': (INT, [P, I32, ctypes.POINTER(MateChannel)]),
    'mate_engine_channel_tape': (INT, [P, P, P, P, P]),
    'mate_engine_channel_edges': (INT, [P, I32, ctypes.POINTER(P), ctypes.POINTER(P)]),
    'mate_engine_enable_seat': (INT, [P, I32, I32, I32, P, P, P, P]),
    'mate_engine_step_seated': (INT, [P, IO, TAPE, I32, P]),
    'mate_engine_seat_rows': (INT, [P, IO, P]),
    'mate_engine_enable_messages': (INT, [P, I32, ctypes.POINTER(MateMessageRows)]),
    'mate_engine_route_messages': (INT, [P, I32, I32, P]),
    'mate_engine_message_edges': (INT, [P, I32, ctypes.POINTER(P), ctypes.POINTER(P), ctypes.POINTER(P), ctypes.POINTER(P), ctypes.POINTER(P)]),
    'mate_engine_message_tape': (INT, [P, P, P, P, P]),
    'mate_engine_rollout_greedy': (INT, [P, IO, I32, I32, P]),
    'mate_engine_rollout_versus_greedy': (INT, [P, I32, IO, I32, I32, P]),
    'mate_engine_observe': (INT, [P, IO, P]),
    'mate_engine_export_state': (INT, [P, P, P]),
    'mate_engine_import_state': (INT, [P, P, P]),
    'mate_engine_enable_state_rows': (INT, [P, P, I32, P, P]),
    'mate_engine_state_rows': (INT, [P, P, I32, P, P, P]),
    'mate_engine_enable_reward_rows': (INT, [P, ctypes.POINTER(MateRewardRows)]),
    'mate_engine_enable_selection': (INT, [P, I32, P, P, P, P, I32]),
    'mate_engine_disable_selection': (INT, [P]),
    'mate_engine_selection_actions': (INT, [P, ctypes.POINTER(P), ctypes.POINTER(I32)]),
    'mate_engine_step_selected': (INT, [P, IO, TAPE, I32, P]),
    'mate_engine_enable_fragment_rows': (INT, [P, ctypes.POINTER(MateFragmentRows)]),
    'mate_engine_fragment_coefficients': (INT, [P, ctypes.POINTER(P), ctypes.POINTER(I32)]),
    'mate_engine_fragment_rows': (INT, [P, ctypes.POINTER(MateFragmentRows), IO, I32, P]),
    'mate_engine_enable_first_rows': (INT, [P, ctypes.POINTER(MateFirstRows)]),
    'mate_engine_enable_frame_fragments': (INT, [P, ctypes.POINTER(MateFrameFragments)]),
    'mate_engine_frame_fragment': (INT, [P, ctypes.POINTER(MateFrameFragments), IO, I32, I32, P]),
    'mate_engine_enable_episode_records': (INT, [P, I32, P, I64, P]),
    'mate_engine_clear_episode_records': (INT, [P, P]),
    'mate_engine_enable_info_rows': (INT, [P, P, P, P]),
    'mate_engine_info_rows': (INT, [P, P, P, P, P, P]),
    'mate_engine_keep_masks': (INT, [P]),
    'mate_engine_render': (INT, [P, P, I64, I32, P, P, P]),
    'mate_engine_enable_comm_trace': (INT, [P, I32, I32]),
    'mate_engine_comm_trace': (INT, [P, I32, ctypes.POINTER(P), ctypes.POINTER(P)]),
    'mate_engine_set_comm_trace': (INT, [P, I32, P]),
    'mate_engine_lut_read': (INT, [P, I64, I32, P, P, I32, ctypes.POINTER(I32)]),
    'mate_engine_lut_read_outer': (INT, [P, I64, I32, P, P, I32, ctypes.POINTER(I32)]),
    'mate_engine_enable_outer_boundary': (INT, [P, ctypes.POINTER(I32)]),
    'mate_engine_lut_write': (INT, [P, I64, I32, P, P, I32]),
    'mate_engine_lut_write_outer': (INT, [P, I64, I32, P, P, I32]),
    'mate_engine_soft_coverage': (INT, [P, P, P, P, P]),
    'mate_engine_rebuild_luts': (INT, [P, P]),
    'mate_engine_idle_steps': (INT, [P, ctypes.POINTER(I64)]),
    'mate_engine_kernel_time': (INT, [P, I32, F64P, ctypes.POINTER(I64)]),
    'mate_engine_last_flow': (INT, [P]),
    'mate_engine_block_alloc': (INT, [I32, I64, ctypes.POINTER(P)]),
    'mate_engine_block_free': (INT, [P]),
    'mate_engine_block_probe': (INT, [I32, P, I64, I32, I32, P, F64P]),
    'mate_engine_set_store_form': (INT, [P, I32]),
    'mate_engine_memory_hold': (INT, [I32, I64, ctypes.POINTER(P)]),
    'mate_engine_memory_release': (INT, [P]),
    'mate_engine_hbm_probe': (INT, [I32, P, P, I64, I32, P, F64P]),
    'mate_engine_set_sub_wave': (INT, [P, I32, ctypes.POINTER(I32)]),
}
EXPORTED_SYMBOLS = tuple(PROTOTYPES)

lib = None


def load():
    """Load the HIP engine; raises if it has not been built (python -m mate_amd.build)."""
    global lib
    if lib is not None:
        return lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f'{LIB_PATH} is missing: build the HIP engine first (python -m mate_amd.build or '
            f'__graft_entry__.build()).  mate_amd has no CPU fallback.')
    # torch first: the engine must bind to the HIP runtime torch already loaded (one runtime per
    # process; loading ROCm's copy before torch's leaves the later one without a device).
    import torch  # noqa: F401
    handle = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = restype, argtypes
    lib = handle
    return lib


class HeldMemory:
    """Physical device memory taken and held, unmapped (``mate_engine_memory_hold``): a spacer between two block candidates."""

    def __init__(self, device_index, nbytes):
        token = ctypes.c_void_p()
        check(load().mate_engine_memory_hold(int(device_index), int(nbytes), ctypes.byref(token)))
        self.token, self._lib = token.value, lib

    def __del__(self):
        token, self.token = getattr(self, 'token', None), None
        if token:
            try:
                self._lib.mate_engine_memory_release(ctypes.c_void_p(token))
            except Exception:
                pass


class ScatteredBlock:
    """Device memory from ``mate_engine_block_alloc`` (2 MiB physical chunks mapped in a shuffled order: what the fused
    rollouts store fastest into, include/mate_engine.h) as a zero-copy torch tensor: ``tensor(dtype, shape)``.  The memory
    lives as long as any tensor made from it."""

    def __init__(self, device_index, nbytes):
        ptr = ctypes.c_void_p()
        check(load().mate_engine_block_alloc(int(device_index), int(nbytes), ctypes.byref(ptr)))
        self.ptr, self.nbytes, self.device_index, self._lib = ptr.value, int(nbytes), int(device_index), lib
        self.__cuda_array_interface__ = {'shape': (self.nbytes,), 'typestr': '|u1', 'data': (self.ptr, False), 'version': 2}

    def store_rate(self, rows_per_step, row_bytes, stream=None):
        """GB/s this block takes in the fused rollouts' store pattern (mate_engine_block_probe); leaves it zeroed."""
        rate = ctypes.c_double()
        check(self._lib.mate_engine_block_probe(self.device_index, ctypes.c_void_p(self.ptr), self.nbytes, int(rows_per_step), int(row_bytes),
                                                stream, ctypes.byref(rate)))
        return rate.value

    def tensor(self, dtype, shape):
        import torch
        flat = torch.as_tensor(self, device=torch.device('cuda', self.device_index))       # keeps a reference to this object
        return flat.view(dtype).view(shape)

    def __del__(self):
        ptr, self.ptr = getattr(self, 'ptr', None), None
        if ptr:
            try:
                import torch
                torch.cuda.synchronize(self.device_index)      # block_free does not wait for launches in flight
                status = self._lib.mate_engine_block_free(ctypes.c_void_p(ptr))
            except Exception:       # interpreter shutdown: the process's memory goes with it
                return
            if status != 0:         # (a finaliser cannot raise: say that device memory may not have come back)
                import warnings
                warnings.warn(f'mate_engine_block_free failed ({status}): {self._lib.mate_engine_last_error().decode()}', RuntimeWarning)


def hbm_rates(device_index, gib=1.0):
    """GB/s of this GPU under the library's own streaming kernels (``mate_engine_hbm_probe``): ``{'copy': read + write bytes of a
    copy, 'fill': write-only (the faster of non-temporal and plain stores), 'read': read-only}`` over two ``gib``-sized buffers, each the
    median of five launches."""
    import torch
    n = int(gib * (1 << 30)) // 16 * 16
    out = {}
    with torch.cuda.device(device_index):
        a = torch.zeros(n, dtype=torch.uint8, device='cuda')
        b = torch.zeros(n, dtype=torch.uint8, device='cuda')
        torch.cuda.synchronize()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for name, mode in (('copy', 0), ('fill', 1), ('read', 2), ('fill', 3)):
            rate = ctypes.c_double()
            check(load().mate_engine_hbm_probe(int(device_index), ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), n, mode, stream, ctypes.byref(rate)))
            out[name] = max(out.get(name, 0.0), rate.value)
        del a, b
        torch.cuda.empty_cache()
    return out


def check(status):
    if status != 0:
        raise EngineError(status, load().mate_engine_last_error().decode())
