"""cc_relabel_consecutive (csrc/cc_relabel.hip) on every path of k_rl_unique and k_rl_apply, against
oracle.relabel.relabel_consecutive: relabelled volumes and assignment tables bit-exact.

The launch rule, restated from the entry's host code and asserted before the device calls
(test_constants_match_source compares the constants with the sources):

  * both kernels load VW ids per lane: VW = 2 (16-B loads and stores) when the input and the
    output are 16-B aligned, VW = 1 (one id per lane) otherwise;
  * a step is RL_WG * RL_Q * VW = 512 * 8 * VW ids (one trip of a workgroup's loop), a workgroup owns
    per_wg = ceil(steps / 8192) * step consecutive ids: one step up to 8192 steps;
  * a workgroup keeps the ids of its range in an LDS set of EV_LDS = 2048 slots and hands them to
    k_rl_apply as a list; a range of more than 2048 distinct ids cannot (pigeonhole), its list is
    marked overflowed (WGN = ~0u) and k_rl_apply looks every run head up in HBM; a range of fewer
    than EV_LDS_PROBES = 32 ids never overflows;
  * a VW = 2 lane whose second id lies past the end loads and stores one id (the scalar tail)."""
import os
import re

import numpy as np
import pytest

from oracle import relabel as R

RL_WG, RL_Q = 512, 8     # threads of a workgroup, loads per lane and trip
RL_WGS = 8192            # workgroups aimed at
EV_LDS, EV_LDS_PROBES = 2048, 32
RESERVED = np.uint64(2 ** 64 - 1)
GUARD = -7               # fills the elements around a buffer and an output before the call
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'cluster_tools_amd', 'csrc')

TAILS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 16385]


def test_constants_match_source():
    """RL_Q, RL_WG, the 8192 workgroups, EV_LDS and the alignment rule as the sources state them"""
    rl = open(os.path.join(CSRC, 'cc_relabel.hip')).read()
    tp = open(os.path.join(CSRC, 'cc_table_pass.hpp')).read()
    assert int(re.search(r'constexpr int RL_Q = (\d+);', rl).group(1)) == RL_Q
    assert int(re.search(r'#define CC_RL_QA (\d+)', rl).group(1)) == RL_Q       # k_rl_apply: the same trips
    assert int(re.search(r'constexpr int RL_WG = (\d+);', rl).group(1)) == RL_WG
    assert int(re.search(r'constexpr int EV_LDS = (\d+);', tp).group(1)) == EV_LDS
    assert int(re.search(r'constexpr int EV_LDS_PROBES = (\d+);', tp).group(1)) == EV_LDS_PROBES
    assert 'const bool vw2 = ((uintptr_t)labels % 16 == 0) && ((uintptr_t)out % 16 == 0);' in rl
    assert 'step = (int64_t)RL_WG * RL_Q * (vw2 ? 2 : 1), steps = (n + step - 1) / step;' in rl
    assert 'per_wg = ((steps + %d) / %d) * step;' % (RL_WGS - 1, RL_WGS) in rl


def launch(n, d, out):
    """the load width, step, ids per workgroup and workgroups of a call, by the host rule"""
    vw = 2 if d.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 else 1
    step = RL_WG * RL_Q * vw
    steps = -(-n // step)
    per_wg = -(-steps // RL_WGS) * step
    return dict(vw=vw, step=step, steps=steps, per_wg=per_wg, grid=-(-n // per_wg))


def _buffer(shape, unaligned, src=None):
    """(storage, view of `shape` inside it): the view 16-B aligned, or 8-B aligned only; two GUARD
    elements or more on either side; filled from the uint64 array src, or with GUARD"""
    import torch
    n = int(np.prod(shape))
    buf = torch.full((n + 6,), GUARD, dtype=torch.int64, device='cuda')
    off = 3 if unaligned else 2
    view = buf[off:off + n].view(shape)
    assert view.data_ptr() % 16 == (8 if unaligned else 0)
    if src is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(src).view(np.int64)).view(shape))
    return buf, view


def _guards_intact(buf, view):
    off = (view.data_ptr() - buf.data_ptr()) // 8
    return bool((buf[:off] == GUARD).all()) and bool((buf[off + view.numel():] == GUARD).all())


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _pool(rng, k, zero):
    """k sorted sparse ids up to 2^62, 2^64 - 2 the last; with or without 0"""
    ids = np.unique(rng.integers(1, 1 << 62, size=k, dtype=np.int64).astype(np.uint64))
    ids[-1] = np.uint64(2 ** 64 - 2)
    if zero:
        ids[0] = 0
    return ids


def _run_labels(rng, n, pool, max_run=5):
    lens = rng.integers(1, max_run + 1, size=n)
    return pool[np.repeat(rng.integers(0, len(pool), size=n), lens)[:n]].reshape(1, 1, n)


def both_ways(ctx, lab, alignments=((False, False), (False, True), (True, False), (True, True)), expect=None,
              **kw):
    """relabel `lab` out of place for every (input, output) alignment and in place for both, against
    the oracle; `expect` is checked against the launch rule of every call"""
    want, wa = R.relabel_consecutive(lab)
    n = lab.size
    for ua_in, ua_out in alignments:
        ibuf, d = _buffer(lab.shape, ua_in, lab)
        obuf, out = _buffer(lab.shape, ua_out)
        geo = launch(n, d, out)
        assert geo['vw'] == (1 if ua_in or ua_out else 2)
        if expect:
            expect(geo)
        got, table = ctx.relabel_consecutive(d, out=out, **kw)
        assert got is out
        np.testing.assert_array_equal(_host(out), want)
        np.testing.assert_array_equal(table, wa)
        np.testing.assert_array_equal(_host(d), lab)               # the input is left alone
        assert _guards_intact(obuf, out) and _guards_intact(ibuf, d)
    for ua in sorted({a for a, b in alignments if a == b}):
        buf, d = _buffer(lab.shape, ua, lab)
        geo = launch(n, d, d)
        assert geo['vw'] == (1 if ua else 2)
        if expect:
            expect(geo)
        _, table = ctx.relabel_consecutive(d, out=d, **kw)
        np.testing.assert_array_equal(_host(d), want)
        np.testing.assert_array_equal(table, wa)
        assert _guards_intact(buf, d)
    return want, wa


@pytest.mark.gpu
@pytest.mark.parametrize('n', TAILS)
def test_gpu_relabel_tails(ctx, n):
    """Lengths around the load (64 lanes x VW), wave trip (512 x VW), step and workgroup-range
    sizes, with runs of 1..5 ids and one run laid across index 4096 and 8192 (the range ends of
    both widths): all four alignments of input and output out of place, both in place.  An odd
    length ends a 16-B call in the scalar tail; 8193 gives its second workgroup one id.  The
    elements around the output stay untouched."""
    rng = np.random.default_rng(1000 + n)
    pool = _pool(rng, 40, zero=n % 2 == 0)
    lab = _run_labels(rng, n, pool)
    flat = lab.reshape(-1)
    for edge in (4096, 8192):
        if n > edge - 6:
            flat[edge - 6:edge + 7] = pool[3 + edge // 4096]
            assert n <= edge or flat[edge - 1] == flat[edge]

    def expect(geo):
        assert geo['per_wg'] == geo['step'] == 4096 * geo['vw'] and geo['grid'] == -(-n // geo['step'])
    both_ways(ctx, lab, expect=expect)


@pytest.mark.gpu
@pytest.mark.parametrize('zero', [True, False], ids=['zero', 'no_zero'])
def test_gpu_relabel_start_label(ctx, zero):
    """find_labeling.py:106-116: new ids from 0 when 0 occurs, from 1 otherwise; on both load widths"""
    rng = np.random.default_rng(7)
    pool = _pool(rng, 300, zero)
    lab = _run_labels(rng, 2999, pool)
    assert (lab == 0).any() == zero
    _, wa = both_ways(ctx, lab, alignments=((False, False), (True, True)))
    assert wa[0].tolist() == ([0, 0] if zero else [int(pool[0]), 1]) and int(wa[-1, 0]) == 2 ** 64 - 2


def _overflow_labels(zero):
    """5 * 8192 + 37 ids: all distinct and sparse over [0, 8192), [16384, 24576) and from 32768 on,
    runs of five ids over [8192, 16384), one id over [24576, 32768)"""
    rng = np.random.default_rng(17)
    n = 5 * 8192 + 37
    lab = np.unique(rng.integers(1, 1 << 62, size=n + 64, dtype=np.int64).astype(np.uint64))
    assert len(lab) >= n
    lab = rng.permutation(lab)[:n]
    few = _pool(rng, 5, zero)
    lab[8192:16384] = _run_labels(rng, 8192, few, max_run=40).reshape(-1)
    lab[24576:32768] = few[2]
    assert (lab == 0).any() == zero
    return lab.reshape(1, 1, n)


@pytest.mark.gpu
@pytest.mark.parametrize('zero', [True, False], ids=['zero', 'no_zero'])
@pytest.mark.parametrize('unaligned', [False, True], ids=['16B', '8B'])
def test_gpu_relabel_lds_overflow(ctx, unaligned, zero):
    """Three workgroup ranges and more of all-distinct ids -- more than the 2048 LDS slots, so their
    lists overflow (WGN = ~0u) and k_rl_apply looks up in HBM -- beside ranges of at most five ids,
    which cannot overflow and map from LDS: both routes in one launch, on the 16-B and on the
    one-id-per-lane template, out of place and in place, with and without 0."""
    lab = _overflow_labels(zero)
    flat = lab.reshape(-1)

    def expect(geo):
        assert geo['vw'] == (1 if unaligned else 2) and geo['per_wg'] == geo['step']
        distinct = [len(np.unique(flat[b:b + geo['per_wg']])) for b in range(0, lab.size, geo['per_wg'])]
        assert len(distinct) == geo['grid'] >= 6
        assert sum(d > EV_LDS for d in distinct) >= 3 and sum(d < EV_LDS_PROBES for d in distinct) >= 2
    both_ways(ctx, lab, alignments=((unaligned, unaligned),), expect=expect)


@pytest.mark.gpu
@pytest.mark.parametrize('unaligned', [False, True], ids=['16B', '8B'])
@pytest.mark.parametrize('where', ['first', 'in_run', 'last_odd'])
def test_gpu_relabel_reserved_id(ctx, where, unaligned):
    """The id 2^64 - 1 (the free-slot key) at the first voxel, inside a run, and in the last voxel of
    an odd length (the scalar tail of a 16-B call) raises RuntimeError("... reserved"), out of place
    and in place, and writes nothing; the same context then relabels the clean volume."""
    rng = np.random.default_rng(23)
    n = 1025
    pool = _pool(rng, 30, zero=True)
    clean = _run_labels(rng, n, pool)
    clean.reshape(-1)[500:512] = pool[4]
    lab = clean.copy()
    at = {'first': slice(0, 1), 'in_run': slice(504, 507), 'last_odd': slice(n - 1, n)}[where]
    lab.reshape(-1)[at] = RESERVED
    assert n % 2 == 1 and lab.reshape(-1)[503] == lab.reshape(-1)[507] == pool[4]
    ibuf, d = _buffer(lab.shape, unaligned, lab)
    obuf, out = _buffer(lab.shape, unaligned)
    assert launch(n, d, out)['vw'] == (1 if unaligned else 2)
    with pytest.raises(RuntimeError, match='reserved'):
        ctx.relabel_consecutive(d, out=out)
    assert bool((obuf == GUARD).all())
    with pytest.raises(RuntimeError, match='reserved'):
        ctx.relabel_consecutive(d, out=d)
    np.testing.assert_array_equal(_host(d), lab)
    assert _guards_intact(ibuf, d)
    both_ways(ctx, clean, alignments=((unaligned, unaligned),))


@pytest.mark.gpu
@pytest.mark.parametrize('unaligned', [False, True], ids=['16B', '8B'])
def test_gpu_relabel_in_place_two_calls(unaligned):
    """relabel_consecutive(d, out=d, cap_hint=1) with 400 ids: the host table of the first C call
    holds one entry, so that call must report the count and leave d alone (k_rl_apply does not
    run); the second maps d.  A first call that wrote d would make the table list new ids as old
    ones.  Fresh context: k_rl_unique runs twice, k_rl_apply once."""
    from cluster_tools_amd import _lib
    rng = np.random.default_rng(29)
    pool = _pool(rng, 400, zero=False)
    lab = _run_labels(rng, 9001, pool)
    want, wa = R.relabel_consecutive(lab)
    assert len(wa) > 1 and not np.array_equal(wa[:, 0], wa[:, 1])
    buf, d = _buffer(lab.shape, unaligned, lab)
    assert launch(lab.size, d, d)['vw'] == (1 if unaligned else 2)
    with _lib.Context(0) as fresh:
        fresh.set_profiling(1)
        out, table = fresh.relabel_consecutive(d, out=d, cap_hint=1)
        prof = fresh.profile()
    assert out is d
    np.testing.assert_array_equal(table, wa)
    np.testing.assert_array_equal(_host(d), want)
    assert _guards_intact(buf, d)
    assert prof['k_rl_unique']['count'] == 2 and prof['k_rl_apply']['count'] == 1


@pytest.mark.gpu
def test_gpu_relabel_multi_step_ranges(ctx):
    """8194 steps of the one-id-per-lane path (8192 * 4096 + 4096 + 13 ids, 8-B aligned only): more
    than 8192 steps, so every workgroup owns two steps and loops twice, the last one over 13 ids of
    its second step.  The labels are pool[idx] of a sorted pool of 3000 sparse ids, all of which
    occur, so the expected output is idx + start without a unique over the volume; compared on
    the device, out of place and in place."""
    import torch
    n = RL_WGS * 4096 + 4096 + 13
    gen = torch.Generator(device='cuda')
    gen.manual_seed(31)
    m = n // 2
    vals = torch.randint(0, 3000, (m,), device='cuda', generator=gen)
    lens = torch.randint(1, 6, (m,), device='cuda', generator=gen)
    idx = torch.repeat_interleave(vals, lens)[:n]
    del vals, lens
    assert idx.numel() == n and int(torch.bincount(idx, minlength=3000).min()) > 0
    pool = _pool(np.random.default_rng(37), 3000, zero=False)
    assert len(pool) == 3000
    dpool = torch.from_numpy(pool.view(np.int64)).cuda()
    buf, d = _buffer((1, 1, n), True)
    d.view(-1).copy_(dpool[idx])
    expected = (idx + 1).view(1, 1, n)
    obuf, out = _buffer((1, 1, n), False)
    geo = launch(n, d, out)
    assert geo['vw'] == 1 and geo['steps'] == 8194 > RL_WGS and geo['per_wg'] == 2 * geo['step']
    assert geo['grid'] == 4097 and n - (geo['grid'] - 1) * geo['per_wg'] == 4096 + 13
    keep = d.clone()
    _, table = ctx.relabel_consecutive(d, out=out)
    assert torch.equal(out, expected) and torch.equal(d, keep) and _guards_intact(obuf, out)
    np.testing.assert_array_equal(table[:, 0], pool)
    np.testing.assert_array_equal(table[:, 1], np.arange(1, 3001, dtype=np.uint64))
    del out, obuf, keep
    ctx.relabel_consecutive(d, out=d)
    assert torch.equal(d, expected) and _guards_intact(buf, d)
