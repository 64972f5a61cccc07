"""The watershed seeds' definition (include/cc_mi355x.h: cc_local_maxima_seeds,
cc_gaussian_smooth_domains) on the CPU: the candidate / kill statement of tests/_seeds_ref.py
against the plateau definition itself (maxima_brute), the stated edge rules, the smoothing against
oracle.gaussian_smooth, the task's configuration, and the host-side argument checks of the two
entries (no GPU: they precede the first device call)."""
import numpy as np
import pytest
from scipy import ndimage as ndi

import _seeds_ref as SR
from _distance_transform_ref import blocks
from oracle import oracle as O


def quantised(shape, q, seed=0):
    """round(q * normalized gaussian_filter(random, 2)): smooth hills cut into q + 1 levels."""
    f = ndi.gaussian_filter(np.random.default_rng(seed).random(shape), 2)
    return np.round((f - f.min()) / (f.max() - f.min()) * q).astype(np.float32)


@pytest.mark.parametrize('indirect', [False, True])
@pytest.mark.parametrize('q', [3, 8, 1000])
@pytest.mark.parametrize('shape', [(33, 70), (5, 20, 37)])
def test_candidate_kill_equals_plateau_definition(shape, q, indirect):
    f = quantised(shape, q)
    m = SR.maxima(f, indirect)
    np.testing.assert_array_equal(m, SR.maxima_brute(f, indirect))
    lab, n = SR.number(m)
    share = m.mean()
    print('%s q %d indirect %s: %d maxima voxels (%.1f %%), %d seeds' % (shape, q, indirect, m.sum(), 100 * share, n))
    assert 1 <= n <= m.sum() and 0 < share < 0.2
    # numbered 1 .. n by the first raster index of each seed
    first = [np.flatnonzero(lab.ravel() == i)[0] for i in range(1, n + 1)]
    assert first == sorted(first) and set(np.unique(lab)) == set(range(n + 1))


def test_constant_domain_is_all_ones():
    for shape in ((1, 6, 7), (3, 4, 5)):
        for value in (0.0, 2.5, np.inf, -np.inf):
            for indirect in (False, True):
                lab, counts = SR.seeds(np.full(shape, value, dtype=np.float32), None, indirect)
                assert (lab == 1).all() and counts.tolist() == [1]
    lab, counts = SR.seeds(np.zeros((2, 6, 7), dtype=np.float32), (1, 6, 7), True)
    assert (lab == 1).all() and counts.tolist() == [1, 1]


def test_diagonal_plateau_is_one_maximum_and_several_seeds():
    f = np.zeros((1, 5, 5), dtype=np.float32)
    for i in range(1, 4):
        f[0, i, i] = 1
    m8 = SR.maxima(f[0], True)
    assert m8.sum() == 3 and ndi.label(m8, structure=np.ones((3, 3)))[1] == 1
    lab, counts = SR.seeds(f, None, True)
    assert counts.tolist() == [3] and [int(lab[0, i, i]) for i in range(1, 4)] == [1, 2, 3]
    # under the 4-neighbourhood each of them is a maximum of its own: the same seeds
    lab4, counts4 = SR.seeds(f, None, False)
    np.testing.assert_array_equal(lab4, lab)
    # one strictly higher voxel touching one end diagonally kills the whole plateau under 8 only
    f[0, 4, 4] = 2
    lab, counts = SR.seeds(f, None, True)
    assert counts.tolist() == [1] and lab[0, 4, 4] == 1 and lab.sum() == 1
    lab4, counts4 = SR.seeds(f, None, False)
    assert counts4.tolist() == [4]


def test_nan_rules():
    f = np.zeros((1, 5, 7), dtype=np.float32)
    f[0, 2, 3] = np.nan
    f[0, 0, 0] = 1
    for indirect in (False, True):
        m = SR.maxima(f[0], indirect)
        np.testing.assert_array_equal(m, SR.maxima_brute(f[0], indirect))
        # neither the NaN voxel nor its neighbours; the 0 plateau touches a non-candidate 0: no maximum
        assert not m[2, 3] and m[0, 0] and m.sum() == 1
    # a NaN voxel without a neighbour is a candidate, hence a seed
    lab, counts = SR.seeds(np.full((1, 1, 1), np.nan, dtype=np.float32))
    assert lab.tolist() == [[[1]]] and counts.tolist() == [1]
    lab, counts = SR.seeds(np.full((1, 1, 3), np.nan, dtype=np.float32), (1, 1, 1))
    assert lab.ravel().tolist() == [1, 1, 1] and counts.tolist() == [1, 1, 1]
    assert not SR.seeds(np.full((1, 1, 3), np.nan, dtype=np.float32))[0].any()


def test_negative_zero_equals_zero():
    f = np.zeros((1, 4, 6), dtype=np.float32)
    f[0, :, ::2] = -0.0
    assert np.signbit(f).any()
    for indirect in (False, True):
        lab, counts = SR.seeds(f, None, indirect)
        assert (lab == 1).all() and counts.tolist() == [1]
        np.testing.assert_array_equal(SR.maxima(f[0], indirect), SR.maxima_brute(f[0], indirect))


def test_domains_are_independent():
    f = quantised((4, 20, 30), 8, seed=3)
    lab, counts = SR.seeds(f, (2, 8, 16), False)
    for i, bb in enumerate(blocks(f.shape, (2, 8, 16))):
        want, n = SR.number(SR.maxima(f[bb], False))
        np.testing.assert_array_equal(lab[bb], want)
        assert counts[i] == n


def test_smooth_domains_3d_equals_the_oracle_per_block():
    x = (np.random.default_rng(5).random((11, 20, 23)) * 100).astype(np.float32)
    bs = (4, 10, 12)
    got = SR.smooth_domains(x, bs, 0.7, apply_2d=False)
    for bb in blocks(x.shape, bs):
        np.testing.assert_array_equal(got[bb].view(np.uint32), O.gaussian_smooth(x[bb], 0.7).view(np.uint32))
    # 2-D: every slice on its own, the z extent free
    got2 = SR.smooth_domains(x, (1, 10, 12), 0.7, apply_2d=True)
    np.testing.assert_array_equal(got2, SR.smooth_domains(x, bs, 0.7, apply_2d=True))
    assert (got2 != got).any()
    with pytest.raises(ValueError):
        SR.smooth_domains(x, (4, 10, 2), 0.7, apply_2d=True)


def test_task_config():
    """Fails on the parent commit: the task does not exist there."""
    from cluster_tools_amd.watershed import WatershedSeedsLocal, WatershedSeedsBase, DistanceTransformLocal
    from cluster_tools_amd.watershed.seeds import check_config
    assert issubclass(WatershedSeedsLocal, WatershedSeedsBase)
    cfg = WatershedSeedsLocal.default_task_config()
    dt = DistanceTransformLocal.default_task_config()
    assert all(cfg[k] == v for k, v in dt.items())
    assert (cfg['apply_ws_2d'], cfg['sigma_seeds'], cfg['non_maximum_suppression']) == (True, 2., False)
    check_config(cfg, (9, 70, 131), (4, 32, 64))
    with pytest.raises(NotImplementedError):
        check_config(dict(cfg, non_maximum_suppression=True), (9, 70, 131), (4, 32, 64))
    with pytest.raises(NotImplementedError):
        check_config(dict(cfg, halo=[0, 2, 2]), (9, 70, 131), (4, 32, 64))
    with pytest.raises(ValueError):
        check_config(dict(cfg, pixel_pitch=[2, 1, 1]), (9, 70, 131), (4, 32, 64))
    # ids stay below 2^32 - 1 (cc_watershed_from_seeds): 256 blocks of 2^24 voxels reach it
    check_config(cfg, (1024 - 64, 2048, 2048), (64, 512, 512))
    with pytest.raises(ValueError):
        check_config(cfg, (1024, 2048, 2048), (64, 512, 512))


def test_unique_block_ids_match_the_restatement():
    from cluster_tools_amd.utils import volume_utils as vu
    from cluster_tools_amd.watershed.seeds import unique_block_ids
    shape, bs = (5, 20, 30), (2, 8, 16)
    f = quantised(shape, 1000, seed=7)
    blocking = vu.Blocking([0, 0, 0], list(shape), list(bs))
    for apply_2d in (True, False):
        lab, counts = SR.seeds(f, (1,) + bs[1:] if apply_2d else bs, apply_2d)
        want = SR.unique_ids(lab, counts, shape, bs, apply_2d)
        c = counts.reshape(shape[0], blocking.blocksPerAxis[1], blocking.blocksPerAxis[2]) if apply_2d else counts
        for b, bb in enumerate(blocks(shape, bs)):
            np.testing.assert_array_equal(unique_block_ids(lab, c, blocking, b, apply_2d), want[bb])
        ids = want[want != 0]
        assert (want != 0).sum() == (lab != 0).sum()
        # a seed keeps one id, two seeds never share one
        assert len(np.unique(ids)) == counts.sum()


def test_abi_rejects_bad_arguments_on_the_host():
    """Both entries refuse invalid arguments with the library's error code and a message before
    any device call: no context and no device memory exist here."""
    from cluster_tools_amd import _lib
    L = _lib.load()
    assert 'cc_local_maxima_seeds' in _lib.EXPORTS and 'cc_gaussian_smooth_domains' in _lib.EXPORTS

    def i64(a):
        return np.ascontiguousarray(np.asarray(a, dtype=np.int64))

    def seeds(shape, ds, values=None, out=None):
        s, d = i64(shape), i64(ds)
        rc = L.cc_local_maxima_seeds(None, values, s.ctypes.data, d.ctypes.data, 0, out, None)
        return rc, L.cc_last_error().decode()

    for name, args in {'zero domain': ((4, 8, 8), (4, 0, 8)), 'negative domain': ((4, 8, 8), (-1, 8, 8)),
                       'negative shape': ((4, -8, 8), (4, 8, 8)), 'axis': ((4, 8, 2 ** 31), (4, 8, 8)),
                       'domain of 2^32 voxels': ((2 ** 11, 2 ** 11, 2 ** 10), (2 ** 11, 2 ** 11, 2 ** 10))}.items():
        rc, msg = seeds(*args)
        assert rc == -1 and 'local_maxima_seeds' in msg and 'NULL argument' not in msg, (name, rc, msg)
    # an output that overlaps the input (addresses only: nothing is read)
    rc, msg = seeds((4, 8, 8), (4, 8, 8), values=0x10000, out=0x10000 + 4 * 255)
    assert rc == -1 and 'overlap' in msg
    rc, msg = seeds((4, 8, 8), (4, 8, 8), values=0x10000, out=0x10000 + 4 * 256)
    assert rc == -1 and 'NULL argument' in msg          # valid: as far as the missing context
    assert seeds((4, 0, 8), (4, 8, 8))[0] == 0           # a zero dimension: done before anything is needed

    def smooth(shape, bs, apply_2d, sigma):
        s, b = i64(shape), i64(bs)
        rc = L.cc_gaussian_smooth_domains(None, None, s.ctypes.data, b.ctypes.data, apply_2d, float(sigma), None)
        return rc, L.cc_last_error().decode()

    assert smooth((4, 8, 8), (4, 8, 8), 1, 2.0)[0] == -1
