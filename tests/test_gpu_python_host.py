"""The Python host's cached argument blocks and declared state on the device (host section): whatever re-homes or replaces an
output tensor drops the cached MateStepIO structures, and detaching a feature returns the engine to what __init__ declared.  Every
comparison is bit for bit against a twin engine (same scenario, seed and calls) that never took the detour.  MATE-4v2-9 x 8, f32 rows."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, SEED = 8, 23


def _engine(policies=False):
    from mate_amd.config import read_config
    from mate_amd.engine import Engine
    eng = Engine(read_config('MATE-4v2-9.yaml'), N, seed=SEED, obs_dtype=torch.float32)
    if policies:
        eng.enable_policies()
    eng.reset()
    return eng


def _outputs(eng):
    return eng.camera_obs, eng.target_obs, eng.scalars, eng.masks


def _assert_same_bits(got, want):
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
    assert any(bool(a.any()) for a in got)      # (not a comparison of two untouched buffers)


def test_staging_the_outputs_drops_the_cached_argument_blocks():
    eng, twin = _engine(), _engine()
    for e in (eng, twin):
        e.step_random(want_masks=True)      # (fills step_random's cache)
    before = [t.data_ptr() for t in _outputs(eng)]
    eng.stage_outputs()
    assert all(t.data_ptr() != p for t, p in zip(_outputs(eng), before))
    for e in (eng, twin):
        e.reset()
        e.step_random(want_masks=True)
    _assert_same_bits(_outputs(eng), _outputs(twin))


def test_attaching_reward_rows_drops_the_cached_argument_blocks():
    eng, twin = _engine(), _engine()
    for e in (eng, twin):
        e.step_random(want_masks=True)
    eng.enable_reward_rows(camera=({'raw_reward': 1.0, 'num_tracked': 0.5}, 'none'), target=({'raw_reward': 1.0}, 'mean'))
    assert eng._random_io == {}
    for e in (eng, twin):
        e.step_random(want_masks=True)
    _assert_same_bits(_outputs(eng), _outputs(twin))


def test_a_rollout_reservation_that_grows_drops_the_cached_argument_blocks():
    eng, twin = _engine(), _engine()
    twin.reserve_rollout(5, want_masks=True)
    held = None
    for steps in (2, 5):
        got, want = eng.rollout_random(steps, want_masks=True), twin.rollout_random(steps, want_masks=True)
        if steps == 2:
            held = eng._rollout['scalars'].data_ptr()
    assert eng._rollout['steps'] == 5 and eng._rollout['scalars'].data_ptr() != held and set(eng._rollout['_calls']) == {(5, True)}
    _assert_same_bits(got + (eng._rollout['masks'][:5],), want + (twin._rollout['masks'][:5],))


FEATURES = {
    'state_rows': (('state', 'state_normalized'),
                   lambda eng: eng.enable_state_rows(normalize=True), lambda eng: eng.disable_state_rows()),
    'reward_rows': (('camera_reward_rows', 'target_reward_rows', 'camera_reward_terms', 'target_reward_terms', 'reward_coefficients', 'reward_accumulate'),
                    lambda eng: eng.enable_reward_rows(camera=({'raw_reward': 1.0}, 'none'), target=({'is_tracked': 1.0}, 'sum'), accumulate=True, terms=True),
                    lambda eng: eng.disable_reward_rows()),
    'selection': (('selection', 'selection_actions', 'selection_metrics', 'selection_frames', 'action_mask', 'multi_selection', 'selection_accumulate'),
                  lambda eng: eng.enable_selection(multi_selection=True, accumulate=True), lambda eng: eng.disable_selection()),
    'fragment_rows': (('fragment_obs', 'fragment_rewards', 'fragment_done', 'fragment_frames', 'fragment_info', 'fragment_shaped',
                       'fragment_coefficients', 'fragment_team', 'fragment_frame_skip', '_fragment_masks', 'fragment_first_rows',
                       'fragment_first_scalars', 'fragment_final_obs', 'fragment', 'fragment_restarted'),
                      lambda eng: eng.enable_fragment_rows('camera', 3, shaping=({'raw_reward': 1.0, 'num_tracked': 1.0}, 'none'), first_rows=True, final_obs=True),
                      lambda eng: eng.disable_fragment_rows()),
}


@pytest.mark.parametrize('feature', sorted(FEATURES))
def test_detaching_returns_to_the_declared_state(feature):
    names, enable, disable = FEATURES[feature]
    policies = feature in ('selection', 'fragment_rows')
    eng, twin = _engine(policies), _engine(policies)
    fresh = {name: getattr(twin, name) for name in names}
    assert all(value is None or (value in (0, False) and not isinstance(value, torch.Tensor)) for value in fresh.values()), fresh
    enable(eng)
    attached = {name: getattr(eng, name) for name in names}
    assert all(attached[name] is not None and (isinstance(attached[name], (torch.Tensor, dict)) or attached[name] != fresh[name])
               for name in names), attached
    disable(eng)
    for name in names:
        value = getattr(eng, name)
        assert type(value) is type(fresh[name]) and value == fresh[name], (name, value, fresh[name])
    for e in (eng, twin):
        e.step_random(want_masks=True)
    _assert_same_bits(_outputs(eng), _outputs(twin))
