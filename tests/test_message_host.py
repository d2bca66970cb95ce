"""Host-side tests of the learner's messages through the team's channel (csrc/message_rows.hpp), no GPU: the NumPy router of tests/message_ref.py against
what the reference's own send_messages / receive_messages / step recorded under its channel wrappers (tests/golden/message_*.npz,
tests/golden/make_message_golden.py); the tag rule of the counts; the C ABI's prototypes; the draws' stream; the refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import golden_util as G
import message_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = {      # name -> (no_communication, range_limit, dropout_rate, filtering)
    'message_4v8-9_nocomm_target': ('target', -1.0, 0.0, False), 'message_4v8-9_drop30': ('none', -1.0, 0.3, True), 'message_4v8-9_drop70': ('none', -1.0, 0.7, True),
    'message_4v8-9_range1400': ('none', 1400.0, 0.0, True), 'message_8v8-9_range1000': ('none', 1000.0, 0.0, True),
    'message_8v8-9_range1000_drop30': ('none', 1000.0, 0.3, True),
}
CALLS = {'enable_messages': 3, 'route_messages': 4, 'message_edges': 7, 'message_tape': 5}


def channel_of_fixture(fx, team):
    """The keywords of Engine.set_channel for `team` (0 / 1) of a message fixture, or None where the chain leaves the team alone."""
    no_comm, limit, rate = str(fx['channel/no_communication']), float(fx['channel/range_limit']), float(fx['channel/dropout_rate'])
    disabled = no_comm in ('both', ('camera', 'target')[team])
    if not disabled and limit < 0 and rate == 0.0:
        return None
    return {'disabled': disabled, 'range_limit': limit if limit >= 0 else None, 'dropout_rate': rate}


@pytest.mark.parametrize('name', sorted(FIXTURES))
def test_message_ref_reproduces_the_recorded_reference(name):
    """Every recorded round: who received what (the inbox in sender order, zeros elsewhere), sent and delivered; every step: the per-step edges ahead of
    step(), the episode's totals behind it, the two sums of `info` -- exactly, through the episode end and the reset.  The coverage the recorder accepted
    the seed for is there."""
    fx = G.load(name + '.npz')
    assert (str(fx['channel/no_communication']), float(fx['channel/range_limit']), float(fx['channel/dropout_rate'])) == FIXTURES[name][:3]
    T, M = len(fx['step/done']), int(fx['msg/width'])
    assert 20 <= T <= 40 and M == 4 and int(fx['step/done'].sum()) == 1 and list(np.unique(fx['step/episode'])) == [0, 1]
    assert set(int(k) for k in fx['msg/rounds']) == {0, 1, 2}
    for team, tag in enumerate(('cam', 'tgt')):
        n = int(fx['num_cameras'] if team == 0 else fx['num_targets'])
        channel = channel_of_fixture(fx, team)
        book = R.Counts(1, n)
        off = ~np.eye(n, dtype=bool)
        kept = dropped = twice = 0
        for s in range(T):
            rounds = int(fx['msg/rounds'][s])
            for k in range(rounds):
                sent = fx[f'msg/{tag}_sent'][s, k]
                address = None if fx['msg/broadcast'][s, k] else fx[f'msg/{tag}_address'][None]
                assert address is not None or sent.all()
                keep = R.verdict(channel, fx[f'msg/{tag}_u'][s, k][None], fx[f'msg/{tag}_xy'][s][None], (1, n, n))
                inbox, sent_, delivered = R.route(fx[f'msg/{tag}_payload'][s, k][None], address, True, keep)
                assert np.array_equal(sent_[0], sent) and np.array_equal(delivered[0], fx[f'msg/{tag}_delivered'][s, k]), (tag, s, k)
                assert np.array_equal(inbox[0], fx[f'msg/{tag}_inbox'][s, k]), (tag, s, k)
                if fx['msg/broadcast'][s, k]:      # ... and the per-sender form of the same call
                    again = R.route(fx[f'msg/{tag}_payload'][s, k][None, :, 0, :], None, False, keep)
                    assert all(np.array_equal(a, b) for a, b in zip(again, (inbox, sent_, delivered)))
                book.update(s, int(fx['step/episode'][s]), delivered)
                kept += int((delivered[0] != 0)[off].sum())
                dropped += int(((sent != 0) & (delivered[0] == 0))[off].sum())
            if rounds:
                assert np.array_equal(book.step_edges[0], fx[f'msg/{tag}_step_edges'][s]), (tag, s)
                assert np.array_equal(book.total_edges[0] + book.step_edges[0], fx[f'msg/{tag}_total_edges'][s]), (tag, s)
                assert np.array_equal(book.agent_edges[0, :, 0], fx[f'msg/{tag}_out'][s]) and np.array_equal(book.agent_edges[0, :, 1], fx[f'msg/{tag}_in'][s]), (tag, s)
                if s and fx['step/episode'][s] == fx['step/episode'][s - 1]:
                    assert np.array_equal(book.total_edges[0], fx[f'msg/{tag}_total_edges'][s - 1]), (tag, s)      # what step() left behind the step before
                else:
                    assert not book.total_edges.any()
            else:
                assert not fx[f'msg/{tag}_step_edges'][s].any()
            twice += int((fx[f'msg/{tag}_step_edges'][s] == 2).sum())
        assert twice > 0 or (channel is not None and channel['disabled'])    # two rounds of a pair within one step
        if FIXTURES[name][3]:
            assert kept >= 3 and dropped >= 3, (tag, kept, dropped)
        elif channel is not None:
            assert kept == 0 and dropped > 0
        else:
            assert dropped == 0 and kept > 0
    for key in fx:
        assert fx[key].dtype.kind in 'fiubU', key                           # arrays and names only
    assert os.path.getsize(os.path.join(G.GOLDEN_DIR, name + '.npz')) < 1 << 20


def test_tag_rule_of_the_counts():
    """A tick other than the tag's folds step_edges into total_edges, an episode other than the tag's zeroes both, an environment that is not live keeps
    everything, cleared tags zero both at the next update."""
    one = np.ones((3, 2, 2), dtype=np.int8)
    book = R.Counts(3, 2)
    book.update([5, 5, 5], [1, 1, 1], one).update([5, 5, 5], [1, 1, 1], one)
    assert (book.step_edges == 2).all() and not book.total_edges.any() and (book.agent_edges == 4).all()
    book.update([6, 6, 6], [1, 2, 1], one, live=[True, True, False])
    assert (book.step_edges[0] == 1).all() and (book.total_edges[0] == 2).all()          # folded
    assert (book.step_edges[1] == 1).all() and not book.total_edges[1].any()             # a new episode
    assert (book.step_edges[2] == 2).all() and not book.total_edges[2].any() and book.tick[2] == 5      # skipped
    book.clear_tags()
    book.update([6, 6, 6], [1, 2, 1], 0 * one)
    assert not book.step_edges.any() and not book.total_edges.any() and not book.agent_edges.any()


def test_encoded_payloads_tell_rows_apart():
    for pairwise in (False, True):
        values = R.encoded_payload(5, 3, 6, pairwise, np.float32, first_env=2)
        assert values.shape == ((5, 3, 3, 6) if pairwise else (5, 3, 6)) and len(np.unique(values)) == values.size
    inbox, sent, delivered = R.route(R.encoded_payload(2, 3, 4, False, np.float64), None, False, np.ones((2, 3, 3), dtype=bool))
    assert sent.all() and delivered.all() and np.array_equal(inbox[1, 2, 0], R.encoded_payload(2, 3, 4, False, np.float64)[1, 0])


def test_header_prototypes_and_exports_agree():
    from mate_amd import _native
    with open(os.path.join(ROOT, 'include', 'mate_engine.h')) as fh:
        header = fh.read()
    assert re.search(r'#define\s+MATE_ABI_VERSION\s+1\b', header)
    for call, arity in CALLS.items():
        assert 'mate_engine_' + call in _native.EXPORTED_SYMBOLS
        assert len(_native.PROTOTYPES['mate_engine_' + call][1]) == arity
        declared = re.search(r'\bint mate_engine_%s\(([^;]*)\);' % call, header).group(1)
        assert declared.count(',') == arity - 1, call
    declared = re.search(r'typedef struct \{([^}]*)\} mate_message_rows;', header).group(1)
    members = [re.search(r'(\w+)$', d.strip()).group(1) for part in declared.split(';') if part.strip() for d in part.split(',')]
    assert members == [name for name, _ in _native.MateMessageRows._fields_] == ['width', 'pairwise', 'payload_dev', 'address_dev', 'inbox_dev']
    assert ctypes.sizeof(_native.MateMessageRows) == 32
    lib = ctypes.CDLL(_native.LIB_PATH)
    for call in CALLS:
        assert hasattr(lib, 'mate_engine_' + call)
    lib.mate_engine_abi_version.restype = ctypes.c_int
    assert lib.mate_engine_abi_version() == 1
    from mate_amd.engine import Engine, EngineGroups
    assert Engine.MESSAGE_EDGES == R.EDGE_NAMES
    for method in ('enable_messages', 'route_messages', 'message_edges', 'message_tape'):
        assert callable(getattr(Engine, method)) and callable(getattr(EngineGroups, method))


def test_sources_are_in_the_digest_and_the_stream_is_new():
    """(The digest: tests/test_unit_resources.py.)"""
    csrc = os.path.join(ROOT, 'mate_amd', 'csrc')
    with open(os.path.join(csrc, 'message_rows.hpp')) as fh:
        text = fh.read()
    assert [int(v) for v in re.findall(r'S_MSG\w* = (\d+)', text)] == [R.S_MSG_DROP] == [28]
    assert '#include "channel_rows.hpp"' in text and 'channel_verdict' in text
    taken = []
    for unit in sorted(os.listdir(csrc)):
        if unit != 'message_rows.hpp':
            with open(os.path.join(csrc, unit)) as fh:
                taken += [int(v) for v in re.findall(r'\bS_[A-Z_]+ = (\d+)', fh.read())]
    assert 28 not in taken and max(taken) == 27                                # a stream id no other draw uses
    with open(os.path.join(csrc, 'message_kernels.hip')) as fh:
        kernel = fh.read()
    assert 'channel_verdict(' in kernel and 'bool channel_verdict' not in kernel + text      # included, not restated
    assert R.draw_key(3, 1, 7, 15) == 3 << 12 | 1 << 8 | 7 << 4 | 15


def test_python_level_argument_rules_need_no_device():
    from mate_amd.environment import BatchedMultiAgentTracking
    for kw in (dict(camera_messages=0), dict(target_messages=-2), dict(camera_messages=2.5), dict(target_messages=True)):
        with pytest.raises((ValueError, AssertionError)):
            BatchedMultiAgentTracking('MATE-4v8-9.yaml', num_envs=2, **kw)


def test_refusals_that_need_no_device():
    """The null-engine row of the refusal table, through ctypes (every other row needs an engine: tests/test_gpu_messages.py)."""
    from mate_amd import _native
    lib = _native.load()
    assert lib.mate_engine_enable_messages(None, 0, None) == -1          # MATE_EINVAL: null engine
    assert lib.mate_engine_route_messages(None, 1, 0, None) == -1
    assert lib.mate_engine_message_edges(None, 0, None, None, None, None, None) == -1
    assert lib.mate_engine_message_tape(None, None, None, None, None) == -1
    assert 'null engine' in lib.mate_engine_last_error().decode()
