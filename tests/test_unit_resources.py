"""The resource records of the build's translation units (mate_amd/build.py: UNITS; mate_amd/lib/kernel_resources*.json) and the source
digest, in one place.  kernel_resources.json is pinned to the parent build's, so a new kernel arrives in a unit of its own with a record
of its own: one row in build.UNITS and one entry in EXPECT below.  Every record: no private scratch memory, no dynamic stack, the spill
figures it is held to, the kernels it must hold, and no kernel of any other record.  Needs the built library, no GPU."""
import functools
import glob
import itertools
import json
import os
import re
import shutil

import pytest

from mate_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'mate_amd', 'lib')
CSRC = os.path.join(ROOT, 'mate_amd', 'csrc')
BOTH_SPILLS = ('SGPRs Spill', 'VGPRs Spill')

# Per record.  sources: the units that report into it.  spills: the figures that must be 0.  kernels: name part -> how many kernels carry
# it (None: at least one).  closed: every kernel carries one of the parts, so the counts are the whole record.  figures / names: further
# conditions on each kernel's figures and on the set of names.
EXPECT = {
    # (its names and figures, one by one: tests/test_kernel_resources.py; occupancy: test_host_logic.py)
    'kernel_resources.json': dict(sources={'mate_engine.hip', 'shape_group.hip'}, spills=(), kernels={}, closed=False),
    # (a pass over one action pair per lane: nowhere near a register limit)
    'kernel_resources_opponents.json': dict(sources={'opponent_kernels.hip'}, spills=BOTH_SPILLS, kernels={'heuristic_drift_kernel': None, 'heuristic_camera_kernel': 1}, closed=False,
                                            figures=lambda r: r['VGPRs'] <= 128 and r['Occupancy'] >= 4),
    # (one instantiation per form of the row stores, both inside the register budget of four waves per SIMD)
    'kernel_resources_headline.json': dict(sources={'headline_kernels.hip'}, spills=('VGPRs Spill',), kernels={'headline_rollout_kernel': 2}, closed=True,
                                           figures=lambda r: r['VGPRs'] <= 128 and r['Occupancy'] == 4),
    'kernel_resources_episodes.json': dict(sources={'episode_kernels.hip'}, spills=BOTH_SPILLS, kernels={'episode_rows_kernel': 1}, closed=True),
    'kernel_resources_info.json': dict(sources={'info_kernels.hip'}, spills=BOTH_SPILLS, kernels={'info_rows_kernel': None}, closed=True),
    'kernel_resources_scripted.json': dict(sources={'scripted_kernels.hip'}, spills=BOTH_SPILLS, kernels={'scripted_opponent_kernel': 1}, closed=True),
    # (f32 and f64 observations, the generic shape)
    'kernel_resources_channel.json': dict(sources={'channel_kernels.hip'}, spills=BOTH_SPILLS, kernels={'greedy_channel_kernel': 2}, closed=True),
    'kernel_resources_seat.json': dict(sources={'seat_kernels.hip'}, spills=BOTH_SPILLS, kernels={'greedy_seat_kernel': 2, 'seat_rows_kernel': 2}, closed=True),
    # (f32 and f64 payloads: the template argument behind the mangled name)
    'kernel_resources_message.json': dict(sources={'message_kernels.hip'}, spills=BOTH_SPILLS, kernels={'message_rows_kernel': 2}, closed=True,
                                          names=lambda names: {n[n.index('message_rows_kernel'):][19:21] for n in names} == {'Id', 'If'}),
}
# a name part that no record but its own may hold
OWN_PARTS = {'heuristic_drift': 'kernel_resources_opponents.json', 'info_rows_kernel': 'kernel_resources_info.json'}
# what the units' own tests listed one by one
SOURCES = ('opponent_rows.hpp', 'headline_kernels.hpp', 'episode_rows.hpp', 'info_rows.hpp', 'attached_tile.hpp', 'scripted_rows.hpp', 'channel_rows.hpp',
           'seat_rows.hpp', 'message_rows.hpp', 'message_host.inc', 'mate_engine.h')


@functools.lru_cache(maxsize=None)
def _load(record):
    path = os.path.join(LIB, record)
    assert os.path.exists(path), 'run __graft_entry__.build() first'
    with open(path) as fh:
        return json.load(fh)


@pytest.mark.parametrize('record', sorted(EXPECT))
def test_no_kernel_needs_scratch_a_stack_or_a_spill(record):
    kernels = _load(record)
    assert kernels, record
    for name, r in kernels.items():
        assert r['ScratchSize'] == 0 and r['Dynamic Stack'] == 'False', (name, r)
        assert all(r[figure] == 0 for figure in EXPECT[record]['spills']), (name, r)


@pytest.mark.parametrize('record', sorted(EXPECT))
def test_the_record_holds_its_kernels(record):
    expect, kernels = EXPECT[record], _load(record)
    for part, count in expect['kernels'].items():
        found = sum(part in name for name in kernels)
        assert found >= 1 if count is None else found == count, (part, sorted(kernels))
    if expect['closed']:
        assert all(any(part in name for part in expect['kernels']) for name in kernels), sorted(kernels)
        if None not in expect['kernels'].values():
            assert len(kernels) == sum(expect['kernels'].values()), sorted(kernels)
    for name, r in kernels.items():
        assert expect.get('figures', lambda r: True)(r), (name, r)
    assert expect.get('names', lambda names: True)(set(kernels)), sorted(kernels)


def test_every_pair_of_records_names_disjoint_kernels():
    for a, b in itertools.combinations(sorted(EXPECT), 2):
        assert not set(_load(a)) & set(_load(b)), (a, b)
    for part, own in OWN_PARTS.items():
        assert any(part in name for name in _load(own)), (part, own)
        for record in EXPECT:
            assert record == own or not any(part in name for name in _load(record)), (part, record)


def test_the_engine_record_is_the_parents_byte_for_byte():
    """No existing kernel changed: whatever arrived since came in a unit, and a record, of its own."""
    with open(os.path.join(LIB, 'kernel_resources.json'), 'rb') as a, open(os.path.join(ROOT, 'tests', 'golden', 'kernel_resources_parent.json'), 'rb') as b:
        assert a.read() == b.read()


def test_the_builds_table_these_expectations_and_the_files_agree():
    table = {record for _, _, _, record in build.UNITS}
    assert table == set(EXPECT)
    for record, expect in EXPECT.items():
        assert {source for _, source, _, r in build.UNITS if r == record} == expect['sources'], record
    assert table == {os.path.basename(p) for p in glob.glob(os.path.join(LIB, 'kernel_resources*.json'))}
    assert os.path.basename(build.RESOURCES) == 'kernel_resources.json' and os.path.dirname(build.RESOURCES) == LIB


def test_the_digest_covers_every_source():
    names = [os.path.basename(d) for d in build.DEPS]
    assert len(names) == len(set(names))                       # (the digest names a member by its base name)
    assert set(SOURCES) | set().union(*(expect['sources'] for expect in EXPECT.values())) <= set(names)
    assert build.SRC in build.DEPS and all(os.path.isfile(d) for d in build.DEPS)
    assert build.DEPS[:-1] == sorted(build.DEPS[:-1]) and all(os.path.dirname(d) == CSRC for d in build.DEPS[:-1])      # the same order, so the same digest, on every machine
    assert build.DEPS[-1] == os.path.join(ROOT, 'include', 'mate_engine.h')
    assert all(os.path.splitext(d)[1] in ('.hip', '.hpp', '.h', '.inc') for d in build.DEPS)


def test_every_quoted_include_resolves_to_a_member_of_the_digest():
    members, seen = set(build.DEPS), 0
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name), errors='replace') as fh:
            for included in re.findall(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', fh.read(), flags=re.M):
                seen += 1
                assert os.path.normpath(os.path.join(CSRC, included)) in members, (name, included)
    assert seen > len(build.UNITS)


def test_the_digest_changes_with_a_byte_of_any_member(tmp_path, monkeypatch):
    before = build.source_digest()
    copies = []
    for i, d in enumerate(build.DEPS):
        copies.append(str(tmp_path / ('%02d' % i) / os.path.basename(d)))
        os.makedirs(os.path.dirname(copies[-1]))
        shutil.copyfile(d, copies[-1])
    monkeypatch.setattr(build, 'DEPS', copies)
    assert build.source_digest() == before                     # by content and base name, wherever the tree lies
    seen = {before}
    for path in copies:
        with open(path, 'rb') as fh:
            data = fh.read()
        with open(path, 'wb') as fh:
            fh.write(data[:-1] + bytes([data[-1] ^ 1]))
        seen.add(build.source_digest())
        with open(path, 'wb') as fh:
            fh.write(data)
        assert build.source_digest() == before, path
    assert len(seen) == 1 + len(copies)                        # one digest per changed member, none of them the tree's
