"""Region adjacency graph on the device (cc_region_graph / Context.region_graph): nodes, edges
and edge sizes equal to the numpy restatement (tests/_graph_ref.py, pinned against a brute force by
tests/test_graph_ref.py).

The kernel's tiling (csrc/cc_graph.hip): a wave's tile is GR_R = 16 rows x 64 voxels in x, a
workgroup holds 4 tiles (consecutive along x, then y), and a z chunk has at least 16 planes (at
these sizes exactly 16).  The stripe shape (37, 70, 333) therefore has 3 z chunks, 5 tile rows and
6 tile columns (2 workgroups across x), none of the extents a multiple of the tile."""
import numpy as np
import pytest

import _graph_ref as GR
from test_gpu_size_filter import _dev, _host, table_launches

pytestmark = pytest.mark.gpu

TILE = (16, 16, 64)         # z chunk, rows, x span of a wave's tile


def check(ctx, lab, ignore_label=True, unaligned=False, cap_hint=1 << 20, owned=None):
    lab = np.ascontiguousarray(lab, dtype=np.uint64)
    d = _dev(lab, unaligned)
    want = GR.region_graph(lab, ignore_label, owned)
    got = ctx.region_graph(d, ignore_label=ignore_label, owned=owned, cap_hint=cap_hint)
    GR.assert_graph_equal(got, want)
    np.testing.assert_array_equal(_host(d), lab)               # the input is left alone
    return got


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_gpu_graph_stripes(ctx, axis):
    """L = coordinate + 1 along one axis: every seam between tiles, chunks and workgroups along
    that axis is an edge (c + 1, c + 2) whose size is the area of the plane across it"""
    shape = (37, 70, 333)
    assert all(s > t and s % t for s, t in zip(shape, TILE))
    idx = np.arange(shape[axis], dtype=np.uint64) + 1
    lab = np.broadcast_to(idx.reshape([-1 if a == axis else 1 for a in range(3)]), shape)
    got = check(ctx, lab)
    n = shape[axis]
    area = int(np.prod(shape)) // n
    np.testing.assert_array_equal(got['nodes'], idx)
    np.testing.assert_array_equal(got['edges'], np.stack([idx[:-1], idx[1:]], axis=1))
    np.testing.assert_array_equal(got['sizes'], np.full(n - 1, area, dtype=np.uint64))
    check(ctx, lab, ignore_label=False)


@pytest.mark.parametrize('shape', [(1, 1, 513), (1, 9, 1), (5, 1, 1), (1, 1, 1), (2, 3, 64), (2, 3, 65), (3, 66, 63)])
def test_gpu_graph_degenerate_extents(ctx, shape):
    """extents of 1 (no neighbour in that direction) and extents at the tile's edges"""
    rng = np.random.default_rng(31)
    for ignore in (True, False):
        check(ctx, rng.integers(0, 4, size=shape), ignore)
        check(ctx, np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape), ignore)


def test_gpu_graph_single_label_and_zeros(ctx):
    got = check(ctx, np.full((19, 20, 70), 7, dtype=np.uint64))
    assert got['nodes'].tolist() == [7] and got['edges'].shape == (0, 2) and got['sizes'].shape == (0,)
    got = check(ctx, np.zeros((19, 20, 70), dtype=np.uint64))
    assert got['nodes'].shape == (0,) and got['edges'].shape == (0, 2)
    got = check(ctx, np.zeros((19, 20, 70), dtype=np.uint64), ignore_label=False)
    assert got['nodes'].tolist() == [0] and got['edges'].shape == (0, 2)


def test_gpu_graph_checkerboard_two_ids(ctx):
    """every face of the volume is a face of the one edge"""
    shape = (17, 18, 130)
    z, y, x = np.indices(shape)
    lab = ((z + y + x) % 2 + 3).astype(np.uint64)
    got = check(ctx, lab)
    faces = sum(int(np.prod(shape)) // s * (s - 1) for s in shape)
    assert got['nodes'].tolist() == [3, 4] and got['edges'].tolist() == [[3, 4]] and got['sizes'].tolist() == [faces]


def test_gpu_graph_distinct_ids_table_growth():
    """every voxel its own id (39 780 ids, 114 484 edges of size 1): the workgroups' LDS tables
    are crowded (adds go straight to HBM), and with cap_hint=1 on a fresh context the HBM table
    starts at 2^16 slots, fills up and is grown twice, the pass running again each time; the host
    arrays are too small and a second C call follows"""
    from cluster_tools_amd import _lib
    shape = (17, 18, 130)
    lab = (np.arange(int(np.prod(shape)), dtype=np.uint64) + 1).reshape(shape)
    with _lib.Context(0) as fresh:
        fresh.set_profiling(1)
        got = check(fresh, lab, cap_hint=1)
        n = int(np.prod(shape))
        assert len(got['nodes']) == n == 39780
        assert len(got['edges']) == sum(n // s * (s - 1) for s in shape) == 114484
        assert (got['sizes'] == 1).all()
        # the table's entries are the nodes and the edges; the first call expects 1 + 1 of them
        assert fresh.profile()['k_graph']['count'] == table_launches(n + 114484, [2, n + 114484])
        check(fresh, lab, ignore_label=False, cap_hint=1)


def _voronoi(shape, n_ids, seed, zero_fraction=0.1):
    rng = np.random.default_rng(seed)
    pts = rng.random((n_ids, 3)) * np.array(shape)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'), axis=-1).reshape(-1, 3)
    best = np.full(len(grid), np.inf)
    lab = np.zeros(len(grid), dtype=np.uint64)
    for i, p in enumerate(pts):
        d = ((grid - p) ** 2).sum(axis=1)
        closer = d < best
        best[closer] = d[closer]
        lab[closer] = i + 1
    lab = lab.reshape(shape)
    # zeros in blobs: the cells of every tenth id
    lab[lab % np.uint64(round(1 / zero_fraction)) == 0] = 0
    return lab


@pytest.fixture(scope='module')
def voronoi():
    lab = _voronoi((33, 40, 257), 300, seed=32)
    assert 0.05 < (lab == 0).mean() < 0.2
    return lab


@pytest.mark.parametrize('ignore', [True, False])
def test_gpu_graph_voronoi(ctx, voronoi, ignore):
    got = check(ctx, voronoi, ignore)
    assert len(got['edges']) > 1000 and (0 in got['nodes']) == (not ignore)


def test_gpu_graph_unaligned_base(ctx, voronoi):
    """a view one element past a 16-byte aligned base (the kernel loads one id per lane)"""
    check(ctx, voronoi[:9, :20, :131], unaligned=True)


def test_gpu_graph_id_range(ctx, voronoi):
    """ids up to 2^32 - 2 fit the packed keys; beyond that the volume is relabelled on the device
    and nodes and edges come back in the caller's ids, sorted; 2^64 - 1 is reserved"""
    lab = voronoi[:12, :33, :100].copy()
    top = np.uint64(2 ** 32 - 2)
    packed = np.where(lab != 0, lab + (top - lab.max()), 0).astype(np.uint64)
    assert packed.max() == top
    got = check(ctx, packed)
    assert got['nodes'][-1] == top
    sparse = packed.copy()
    sparse[packed == top] = np.uint64(2 ** 32 - 1)
    sparse[packed == top - np.uint64(1)] = np.uint64(2 ** 32 + 5)
    sparse[packed == top - np.uint64(2)] = np.uint64(2 ** 63 + 11)
    for ignore in (True, False):
        got = check(ctx, sparse, ignore)
        assert got['nodes'][-1] == np.uint64(2 ** 63 + 11)
        order = np.lexsort((got['edges'][:, 1], got['edges'][:, 0]))
        assert (order == np.arange(len(order))).all() and (got['edges'][:, 0] < got['edges'][:, 1]).all()
    bad = lab.copy()
    bad[5, 6, 7] = np.uint64(2 ** 64 - 1)
    with pytest.raises(RuntimeError, match='reserved'):
        ctx.region_graph(_dev(bad))


def test_gpu_graph_owned_pieces(ctx, voronoi):
    """the eight pieces of a volume, each with its one-plane halo, merged == the whole volume"""
    from cluster_tools_amd import _lib
    lab = np.ascontiguousarray(voronoi[:20, :24, :140])
    for ignore in (True, False):
        whole = check(ctx, lab, ignore)
        tables = []
        for begin, end in GR.split_pieces(lab.shape, (9, 17, 71)):
            piece, owned = GR.piece_with_halo(lab, begin, end)
            tables.append(check(ctx, piece, ignore, owned=owned))
        GR.assert_graph_equal(_lib.merge_region_graphs(tables), whole)


def test_gpu_graph_owned_excludes_halo_faces(ctx):
    """faces and ids that lie wholly inside the halo are not counted"""
    lab = np.full((6, 7, 70), 1, dtype=np.uint64)
    lab[5, :, :] = 2          # the halo plane in z: one z edge (1, 2), counted from the owned side
    lab[5, 6, 3:] = 3         # inside the halo plane: the faces (2, 3) lie wholly in the halo
    lab[:, :, 69] = 4         # the halo column in x
    lab[5, :, 69] = 5         # halo only
    got = check(ctx, lab, owned=(5, 6, 69))
    assert got['nodes'].tolist() == [1]
    # (1, 2): the z faces above the 6 x 69 owned columns of plane 4; (1, 4): the x faces right of
    # the 5 x 6 owned voxels of column 68; ids 3 and 5 touch only halo voxels
    assert got['edges'].tolist() == [[1, 2], [1, 4]] and got['sizes'].tolist() == [6 * 69, 5 * 6]
    inner = ctx.region_graph(_dev(lab), owned=(4, 6, 68))
    assert inner['nodes'].tolist() == [1] and inner['edges'].shape == (0, 2)
