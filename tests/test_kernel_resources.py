"""The compiler's figures of every kernel (mate_amd/lib/kernel_resources.json, written by the build) against those of the parent
commit's build.  Needs the built library, no GPU."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_kernel_keeps_the_resources_of_the_parent_build():
    """The same kernel set as tests/golden/kernel_resources_parent.json (a --force build of the parent commit: 281 kernels and the four
    fragment_rows_kernel instances) with identical registers, spills, scratch and occupancy for every one of them; and what the
    attached kernels promised when they came: reward_rows_kernel 48 VGPRs; selection_kernel and fragment_rows_kernel no scratch, no
    dynamic stack, no spills."""
    path = os.path.join(ROOT, 'mate_amd', 'lib', 'kernel_resources.json')
    if not os.path.exists(path):
        pytest.fail('mate_amd/lib/kernel_resources.json is missing: build the engine (python -m mate_amd.build --force)')
    with open(path) as fh:
        now = json.load(fh)
    with open(os.path.join(ROOT, 'tests', 'golden', 'kernel_resources_parent.json')) as fh:
        parent = json.load(fh)
    assert len(parent) == 285
    assert sorted(now) == sorted(parent), (sorted(set(now) - set(parent)), sorted(set(parent) - set(now)))
    changed = {name: (figures, now[name]) for name, figures in parent.items() if now[name] != figures}
    assert not changed, changed
    rewards = [k for k in now if 'reward_rows_kernel' in k]
    selection = [k for k in now if 'selection_kernel' in k]
    fragment = [k for k in now if 'fragment_rows_kernel' in k]
    assert len(rewards) == 2 and len(selection) == 2 and len(fragment) == 4      # <float>, <double>; obs type x row type
    for k in rewards:
        assert now[k]['VGPRs'] == 48 and now[k]['ScratchSize'] == 0 and now[k]['Dynamic Stack'] == 'False' and now[k]['VGPRs Spill'] == 0 and now[k]['SGPRs Spill'] == 0, (k, now[k])
    for k in selection + fragment:
        assert now[k]['ScratchSize'] == 0 and now[k]['Dynamic Stack'] == 'False' and now[k]['VGPRs Spill'] == 0 and now[k]['SGPRs Spill'] == 0, (k, now[k])
