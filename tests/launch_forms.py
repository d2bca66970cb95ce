"""Shared by the launch-form matrices (tests/test_gpu_rims.py, tests/test_gpu_logistics.py): two engines of a shape and the oracle batch
on one natively reset state, byte comparison, and the flows tests/golden/launch_flows.json recorded for the calls."""
import json
import os

import numpy as np
import torch

import gpu_util as U
import rim_scenes as RS

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'launch_flows.json')) as fh:
    GOLDEN = json.load(fh)
# call of tests/test_gpu_rims.py -> call of tools/launch_matrix.py CALL_LIST whose recorded [last_flow, sub_wave] it must run (f32 action tensors there)
RECORDED_CALL = {'observe': 'observe', 'step f32 drawn': 'step', 'step_versus_greedy target': 'step_versus_greedy_target',
                 'rollout_versus_greedy target': 'rollout_versus_greedy_target', 'step_versus_greedy camera': 'step_versus_greedy_camera',
                 'step_random': 'step_random', 'rollout_random': 'rollout_random'}
CALL_ORDER = ['observe'] + [name for name in ('step', 'step_random', 'rollout_random', 'step_greedy', 'step_greedy_tape', 'step_versus_greedy_camera',
                                              'step_versus_greedy_target', 'rollout_greedy', 'rollout_versus_greedy_camera', 'rollout_versus_greedy_target')
                            for _ in range(3)]


def recorded_flow(shape, dtype, mode, split, call, calls=None):
    """[last_flow, sub_wave] tests/golden/launch_flows.json holds for this call (auto_reset = 0), or None where it has no such column.
    `calls`: the caller's own {call: recorded call} in place of RECORDED_CALL."""
    column = '%s %s plain sub_wave=%s' % (shape, dtype, mode)
    columns = GOLDEN['switches'].get('MATE_STEP_SPLIT=%s' % split, {}) if shape == 'MATE-2v4-0' else GOLDEN['flows'].get(shape, {})
    calls = RECORDED_CALL if calls is None else calls
    if column not in columns or call not in calls:
        return None
    return columns[column][CALL_ORDER.index(calls[call])][:2]


def same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


class Matrix:
    """Two engines of a shape (the second one the twin that single-steps what the first one fuses) and the oracle batch, natively
    reset on the same Philox seed; the device's occlusion tables on both sides."""

    def __init__(self, shape, dtype, O, cfg=None):
        from mate_amd.engine import Engine
        self.shape, self.cfg = shape, cfg or RS.config_of(shape)
        self.dtype = dtype
        obs_dtype = torch.float64 if dtype == 'f64' else torch.float32
        self.a, self.b = (Engine(self.cfg, RS.BATCH, seed=RS.SEED, first_env_index=RS.FIRST, obs_dtype=obs_dtype) for _ in range(2))
        for eng in (self.a, self.b):
            eng.enable_policies()
            eng.reset()
        torch.cuda.synchronize()
        self.side = RS.OracleSide(O, shape, self.cfg)
        self.flat0 = self.a.export_state().cpu().numpy()
        self.sd = self.a.state_dict_from(self.flat0.copy())
        for k in U.STATE_KEYS:
            ref = self.side.base[k]
            assert np.array_equal(self.sd[k].reshape(ref.shape), ref), (shape, 'reset', k)
        a = self.a
        self.tables = [[a.lut_read(e, c) for c in range(a.num_cameras)] for e in range(RS.BATCH)]
        self.side.set_tables(self.tables)
        n, Nc, Nt = RS.BATCH, a.num_cameras, a.num_targets
        dev = a.device
        self.no_draws = torch.zeros((n, max(Nc, 1), Nt), dtype=torch.float64, device=dev)
        self.zero_cam = {d: torch.zeros((n, Nc, 2), dtype=d, device=dev) for d in (torch.float32, torch.float64)}
        self.zero_tgt = {d: torch.zeros((n, Nt, 2), dtype=d, device=dev) for d in (torch.float32, torch.float64)}

    def flat_of(self, scene_state):
        """The exported reset state with the scene's fields planted (what Engine.load_state_dict writes)."""
        flat = self.flat0.copy()
        for name, value in scene_state.items():
            off, shape = self.a.export_fields[name]
            k = int(np.prod(shape)) if shape else 1
            flat[:, off:off + k] = np.asarray(value, dtype=np.float64).reshape(RS.BATCH, k)
        return torch.from_numpy(flat)

    @staticmethod
    def plant(eng, flat):
        """The planted state, and the view of it in the engine's mask words: the on-device agents act on the view the last launch
        left (include/mate_engine.h: import_state, then observe() first)."""
        eng.import_state(flat)
        eng.observe()

    def device_state(self, eng):
        sd = eng.state_dict()
        return {k: sd[k] for k in ('tgt_x', 'tgt_y', 'tgt_colliding', 'cam_phi', 'cam_theta')}
