"""The headline's translation unit (csrc/headline_kernels.hip: headline_rollout_kernel, one instantiation per form of the row stores) reports its kernels'
resources apart from the engine's (mate_amd/lib/kernel_resources_headline.json, written by mate_amd/build.py): two kernels, neither with private scratch
memory, a dynamic stack or a spilled vector register, both inside the register budget of four waves per SIMD, and neither named in the other two reports --
kernel_resources.json stays pinned to its own kernels.  Needs the built library, no GPU."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'mate_amd', 'lib')


def _load(name):
    path = os.path.join(LIB, name)
    assert os.path.exists(path), 'run __graft_entry__.build() first'
    with open(path) as fh:
        return json.load(fh)


def test_two_headline_kernels_without_scratch_at_four_waves_per_simd():
    kernels = _load('kernel_resources_headline.json')
    assert len(kernels) == 2 and all('headline_rollout_kernel' in name for name in kernels), sorted(kernels)
    for name, r in kernels.items():
        assert r['ScratchSize'] == 0 and r['Dynamic Stack'] == 'False' and r['VGPRs Spill'] == 0, (name, r)
        assert r['VGPRs'] <= 128 and r['Occupancy'] == 4, (name, r)


def test_the_headline_report_names_no_kernel_of_the_other_reports():
    mine = set(_load('kernel_resources_headline.json'))
    assert mine and not mine & set(_load('kernel_resources.json')) and not mine & set(_load('kernel_resources_opponents.json'))


def test_the_source_digest_covers_the_headline_sources():
    from mate_amd import build
    names = {os.path.basename(d) for d in build.DEPS}
    assert {'headline_kernels.hpp', 'headline_kernels.hip'} <= names
