"""The two host-side helpers every table-pass binding goes through (cluster_tools_amd/_lib.py):
_sized_call -- a call at the capacity hint and once more at exactly the reported count -- and
_relabel_retry -- relabel on CC_ERR_ID_RANGE, call again, map the named arrays back.  No GPU: the
C entries are fakes that record how they were called."""
import numpy as np
import pytest

from cluster_tools_amd import _lib
from cluster_tools_amd._lib import CC_ERR_ID_RANGE, _relabel_retry, _sized_call


def fake_entry(counts, rc=0):
    """attempt(*caps) of a C entry that reports `counts`; .calls: the capacities of every call"""
    calls = []

    def attempt(*caps):
        calls.append(caps)
        return rc, counts, ('buffers of', caps)
    attempt.calls = calls
    return attempt


@pytest.mark.parametrize('hint,first', [(1, 1), (0, 1), (-5, 1), (1024, 1024), (1 << 20, 1 << 20)])
def test_first_attempt_at_the_hint(hint, first):
    a = fake_entry((0,))
    assert _sized_call(a, hint) == (0, ('buffers of', (first,)))
    assert a.calls == [(first,)]


@pytest.mark.parametrize('n', [0, 99, 100])
def test_fitting_count_is_one_attempt(n):
    a = fake_entry((np.uint64(n),))
    assert _sized_call(a, 100) == (0, ('buffers of', (100,)))
    assert a.calls == [(100,)]


@pytest.mark.parametrize('n', [101, 65600])
def test_second_attempt_at_exactly_the_reported_count(n):
    a = fake_entry((np.uint64(n),))
    assert _sized_call(a, 100) == (0, ('buffers of', (n,)))
    assert a.calls == [(100,), (n,)]


@pytest.mark.parametrize('counts,second', [((7, 500), (100, 500)), ((500, 7), (500, 100)), ((101, 300), (101, 300))])
def test_two_capacities_grow_each_to_its_own_count(counts, second):
    a = fake_entry(counts)
    assert _sized_call(a, 100, n_caps=2) == (0, ('buffers of', second))
    assert a.calls == [(100, 100), second]
    b = fake_entry((100, 3))
    _sized_call(b, 100, n_caps=2)
    assert b.calls == [(100, 100)]


@pytest.mark.parametrize('rc', [-1, -2, CC_ERR_ID_RANGE])
def test_error_code_comes_back_after_one_attempt(rc):
    a = fake_entry((10 ** 6,), rc=rc)             # the count of a failed call means nothing
    assert _sized_call(a, 100) == (rc, None)
    assert a.calls == [(100,)]


TABLE = np.array([[10, 1], [2 ** 40, 2], [2 ** 63 + 5, 3]], dtype=np.uint64)      # [old id, new id]


def fake_relabel(seen):
    def relabel(labels):
        seen.append(labels)
        return 'relabelled', TABLE
    return relabel


def graph():
    return {'nodes': np.array([1, 3], dtype=np.uint64), 'edges': np.array([[1, 3], [2, 3]], dtype=np.uint64),
            'sizes': np.array([3, 1], dtype=np.uint64)}


def test_relabel_retry_no_error_maps_nothing():
    seen, calls = [], []

    def call(lab):
        calls.append(lab)
        return 0, graph()
    out = _relabel_retry(call, 'labels', ('nodes', 'edges'), fake_relabel(seen))
    assert calls == ['labels'] and seen == []
    for k, v in graph().items():
        np.testing.assert_array_equal(out[k], v)


def test_relabel_retry_maps_back_only_the_named_arrays():
    seen, calls = [], []

    def call(lab):
        calls.append(lab)
        return (CC_ERR_ID_RANGE, None) if lab == 'labels' else (0, graph())
    out = _relabel_retry(call, 'labels', ('nodes', 'edges'), fake_relabel(seen))
    assert calls == ['labels', 'relabelled'] and seen == ['labels']
    assert out['nodes'].dtype == np.uint64 and out['edges'].dtype == np.uint64
    assert out['nodes'].tolist() == [10, 2 ** 63 + 5]
    assert out['edges'].tolist() == [[10, 2 ** 63 + 5], [2 ** 40, 2 ** 63 + 5]]
    assert out['sizes'].tolist() == [3, 1]         # equal to ids of the table, and left alone
    only_edges = _relabel_retry(call, 'labels', ('edges',), fake_relabel(seen))
    assert only_edges['nodes'].tolist() == [1, 3] and only_edges['edges'].tolist() == out['edges'].tolist()


def test_relabel_retry_empty_result_and_table():
    def call(lab):
        if lab == 'labels':
            return CC_ERR_ID_RANGE, None
        return 0, {'edges': np.zeros((0, 2), dtype=np.uint64)}
    out = _relabel_retry(call, 'labels', ('edges',), lambda lab: ('relabelled', np.zeros((0, 2), dtype=np.uint64)))
    assert out['edges'].shape == (0, 2)


@pytest.mark.parametrize('rc', [-1, -2])
def test_relabel_retry_other_codes_go_through_check(monkeypatch, rc):
    seen, calls, checked = [], [], []

    def check(code):
        checked.append(code)
        raise RuntimeError('libcc_mi355x: the message')
    monkeypatch.setattr(_lib, '_check', check)

    def call(lab):
        calls.append(lab)
        return rc, None
    with pytest.raises(RuntimeError, match='the message'):
        _relabel_retry(call, 'labels', ('edges',), fake_relabel(seen))
    assert calls == ['labels'] and seen == [] and checked == [rc]


def test_relabel_retry_second_failure_goes_through_check(monkeypatch):
    checked = []

    def check(code):
        checked.append(code)
        if code < 0:
            raise RuntimeError('libcc_mi355x: again')
        return code
    monkeypatch.setattr(_lib, '_check', check)
    with pytest.raises(RuntimeError, match='again'):
        _relabel_retry(lambda lab: (CC_ERR_ID_RANGE, None), 'labels', ('edges',), fake_relabel([]))
    assert checked == [CC_ERR_ID_RANGE]
