"""The opponents' translation unit (csrc/opponent_kernels.hip) reports its kernels' resources apart from the engine's
(mate_amd/lib/kernel_resources_opponents.json, written by mate_amd/build.py): no kernel there may need private scratch memory, a
dynamic stack or a spilled register, and none of them may appear in kernel_resources.json, which stays pinned to its own kernels."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'mate_amd', 'lib')


def _load(name):
    path = os.path.join(LIB, name)
    assert os.path.exists(path), 'run __graft_entry__.build() first'
    with open(path) as fh:
        return json.load(fh)


def test_opponent_kernels_need_no_scratch_and_spill_nothing():
    kernels = _load('kernel_resources_opponents.json')
    assert any('heuristic_drift_kernel' in name for name in kernels), sorted(kernels)
    for name, r in kernels.items():
        assert r['ScratchSize'] == 0 and r['Dynamic Stack'] == 'False', (name, r)
        assert r['SGPRs Spill'] == 0 and r['VGPRs Spill'] == 0, (name, r)
        assert r['VGPRs'] <= 128 and r['Occupancy'] >= 4, (name, r)      # (a pass over one action pair per lane: nowhere near a register limit)


def test_the_two_resource_files_name_disjoint_kernels():
    mine, engine = _load('kernel_resources_opponents.json'), _load('kernel_resources.json')
    assert mine and not set(mine) & set(engine)
    assert not any('heuristic_drift' in name for name in engine)


def test_the_source_digest_covers_the_opponents_sources():
    from mate_amd import build
    names = {os.path.basename(d) for d in build.DEPS}
    assert {'opponent_rows.hpp', 'opponent_kernels.inc', 'opponent_kernels.hip'} <= names
