"""Overlaps of two label volumes on the device (cc_label_overlaps / Context.label_overlaps) and the
max-overlap label per node (cc_max_overlaps / Context.node_labels), triple for triple against the
numpy restatement (tests/_node_labels_ref.py, pinned by tests/test_node_labels_ref.py).

The kernel's tiling (csrc/cc_node_labels.hip): a wave item is 512 voxels of one x-row, ws as 8
loads of 64 uint64; the item's labels are fetched by wide loads (8 B per lane for uint8, 16 B for
uint16 / uint32) from the aligned address below the item -- lane 0 fetches one vector more when
the item starts unaligned -- through a wave-private LDS strip; uint64 labels are loaded as ws is.
A workgroup is 4 waves over ceil(rows / 8192) consecutive rows.  The shape (5, 7, 1100) has two
full items and one of 76 voxels per row and one row per workgroup; rows start 4 (uint8) or 8
(uint16) bytes off the load width in turn; (3, 5, 1037) starts its rows at every offset for every
dtype; (93, 89, 7) has 8277 rows, two per workgroup.  The block grid (2, 3, 100) cuts inside
every item."""
import numpy as np
import pytest

import _node_labels_ref as NR
from test_gpu_size_filter import _dev, _host, table_launches

pytestmark = pytest.mark.gpu

ITEM = 512
SHAPE, BLOCK = (5, 7, 1100), (2, 3, 100)
DTYPES = [np.uint8, np.uint16, np.uint32, np.uint64]
SIGNED = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}


def _dev_labels(lab, unaligned=False):
    """the label array on the device in its own width; unaligned: element-aligned, not 16-byte aligned"""
    import torch
    lab = np.ascontiguousarray(lab)
    view = lab.view(np.uint8 if lab.itemsize == 1 else SIGNED[lab.itemsize])
    d = torch.from_numpy(view).cuda()
    if unaligned:
        skip = 1 if lab.itemsize == 8 else 3
        buf = torch.empty(d.numel() + skip, dtype=d.dtype, device='cuda')
        buf[skip:] = d.reshape(-1)
        d = buf[skip:].view(d.shape)
        assert d.data_ptr() % lab.itemsize == 0 and d.data_ptr() % 16 == (skip * lab.itemsize) % 16 != 0
    return d


def _top(dtype):
    """the largest label of a dtype: its top value; 2^64 - 1 is reserved (relabel_consecutive)"""
    return np.uint64(2 ** 64 - 2) if dtype == np.uint64 else np.iinfo(dtype).max


def _host_labels(t, dtype):
    return t.cpu().numpy().view(dtype)


def _volumes(shape, lab_dtype, seed=71, n_ws=40, ws_run=6, lab_block=(2, 2, 37)):
    """ws: runs of ~ws_run voxels along x drawn from n_ws ids (0 among them); labels: coarse
    blocks of 7 ids, the dtype's top value among them"""
    rng = np.random.default_rng(seed)
    ws = rng.integers(0, n_ws, size=(shape[0], shape[1], -(-shape[2] // ws_run))).repeat(ws_run, axis=2)
    ws = np.ascontiguousarray(ws[:, :, :shape[2]]).astype(np.uint64)
    cs = [-(-s // b) for s, b in zip(shape, lab_block)]
    lab = rng.integers(0, 7, size=cs)
    for a, b in enumerate(lab_block):
        lab = lab.repeat(b, axis=a)
    lab = np.ascontiguousarray(lab[:shape[0], :shape[1], :shape[2]]).astype(lab_dtype)
    lab[lab == 6] = _top(lab_dtype)
    return ws, lab


def check(ctx, ws, lab, block_shape=None, ignore_label=None, unaligned=False, cap_hint=1 << 20):
    ws = np.ascontiguousarray(ws, dtype=np.uint64)
    lab = np.ascontiguousarray(lab)
    dw, dl = _dev(ws, unaligned), _dev_labels(lab, unaligned)
    want = NR.label_overlaps(ws, lab, block_shape, ignore_label)
    got = ctx.label_overlaps(dw, dl, block_shape=block_shape, ignore_label=ignore_label, cap_hint=cap_hint)
    NR.assert_overlaps_equal(got, want)
    np.testing.assert_array_equal(_host(dw), ws)                   # the inputs are left alone
    np.testing.assert_array_equal(_host_labels(dl, lab.dtype), lab)
    return got


@pytest.fixture(scope='module')
def main_case():
    """(5, 7, 1100) with blocks (2, 3, 100): two blocks without ws whose labels are a value of
    their own, and ws 0 elsewhere in mixed blocks"""
    ws, lab = _volumes(SHAPE, np.uint8)
    assert SHAPE[2] % ITEM and SHAPE[2] > ITEM and ITEM % BLOCK[2]
    ws[0:2, 0:3, 100:300] = 0
    lab[0:2, 0:3, 100:300] = 77
    assert (ws[2:] == 0).any() and (lab != 77)[ws != 0].all()
    return ws, lab


@pytest.mark.parametrize('ignore', [None, 0, 3])
@pytest.mark.parametrize('dtype', DTYPES)
def test_gpu_node_labels_dtypes(ctx, main_case, dtype, ignore):
    """every label dtype, its top value a label (2^32 - 1 and 2^64 - 2 take the id-range path),
    ignore_label None, 0 and a non-zero value that occurs"""
    ws, lab8 = main_case
    lab = lab8.astype(dtype)
    top = _top(dtype)
    lab[lab8 == 255] = top
    assert (lab == 3).any() and (lab == 0).any() and (lab == top).any()
    got = check(ctx, ws, lab, BLOCK, ignore)
    d = NR.as_dict(got)
    assert int(top) in got['label_ids'].tolist() and (ignore is None or ignore not in got['label_ids'].tolist())
    # the ws-free blocks contribute nothing; the ws-0 voxels of mixed blocks do
    assert (0, 77) not in d and any(w == 0 for w, _ in d)
    assert int(got['counts'].sum()) == int(((lab != ignore) & (lab != 77)).sum() if ignore is not None
                                           else (lab != 77).sum())
    whole = check(ctx, ws, lab, None, ignore)                      # one block: the whole volume
    assert NR.as_dict(whole)[(0, 77)] == 2 * 3 * 200


@pytest.mark.parametrize('dtype', DTYPES)
def test_gpu_node_labels_row_offsets(ctx, dtype):
    """x extent 1037: the rows' labels start at every offset to the load width; aligned and
    unaligned buffers (ws too)"""
    ws, lab = _volumes((3, 5, 1037), dtype, seed=72)
    for unaligned in (False, True):
        check(ctx, ws, lab, (2, 2, 300), None, unaligned=unaligned)
        check(ctx, ws, lab, (2, 2, 300), 0, unaligned=unaligned)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
def test_gpu_node_labels_unaligned_main(ctx, main_case, dtype):
    ws, lab = main_case
    check(ctx, ws, lab.astype(dtype), BLOCK, 0, unaligned=True)


@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 1, 700), (1, 9, 1), (6, 1, 1), (2, 3, 512), (2, 3, 513), (3, 2, 63)])
def test_gpu_node_labels_degenerate_extents(ctx, shape):
    for dtype in DTYPES:
        ws, lab = _volumes(shape, dtype, seed=73, n_ws=4, ws_run=2, lab_block=(1, 2, 3))
        check(ctx, ws, lab, (1, 2, 5), None)
        check(ctx, ws, lab, None, 0)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint64])
def test_gpu_node_labels_two_rows_per_workgroup(ctx, dtype):
    """8277 rows: a workgroup owns two rows, and the blocks (2, 3, 4) cut between them"""
    shape = (93, 89, 7)
    assert shape[0] * shape[1] > 8192
    ws, lab = _volumes(shape, dtype, seed=74, n_ws=30, ws_run=3, lab_block=(5, 4, 2))
    ws[10:20] = 0                                          # planes of ws-free blocks
    check(ctx, ws, lab, (2, 3, 4), 0)
    check(ctx, ws, lab, (2, 3, 4), None)


def test_gpu_node_labels_id_range(ctx, main_case):
    """ids beyond the key packing (ws >= 2^31, labels >= 2^32 - 1): the volumes are relabelled on
    the device and the triples come back in the caller's ids, sorted; the ignore label among the
    out-of-range ids, and absent"""
    ws, lab8 = main_case
    lab = lab8.astype(np.uint64)
    lab[lab8 == 255] = np.uint64(2 ** 32 - 1)
    lab[lab8 == 5] = np.uint64(2 ** 40 + 3)
    lab[lab8 == 4] = np.uint64(2 ** 63 + 9)
    for ignore in (2 ** 40 + 3, 2 ** 63 + 9, 2 ** 50, 0, None):
        got = check(ctx, ws, lab, BLOCK, ignore)
        assert ignore is None or ignore not in got['label_ids'].tolist()
        assert got['label_ids'].max() == (2 ** 63 + 9 if ignore != 2 ** 63 + 9 else 2 ** 40 + 3)
    big = ws.copy()
    big[ws == 7] = np.uint64(2 ** 31)
    big[ws == 8] = np.uint64(2 ** 64 - 2)
    got = check(ctx, big, lab8, BLOCK, 0)                          # ws alone
    assert got['ws_ids'][-1] == np.uint64(2 ** 64 - 2)
    check(ctx, big, lab, BLOCK, 2 ** 40 + 3)                       # both
    lab32 = lab8.astype(np.uint32)
    lab32[lab8 == 255] = 2 ** 32 - 1
    check(ctx, big, lab32, BLOCK, 2 ** 32 - 1)
    check(ctx, ws, lab32 - (lab32 == 2 ** 32 - 1).astype(np.uint32), BLOCK, None)      # 2^32 - 2 fits the packing


def test_gpu_node_labels_crowded_tables():
    """every voxel its own pair (40 800 of them) on a fresh context with cap_hint=1: a row's 3400
    pairs overflow its workgroup's 2048-entry LDS table (adds go straight to HBM), and the HBM
    table starts at 2^16 slots, is more than half full and is grown, the pass running again"""
    from cluster_tools_amd import _lib
    shape = (3, 4, 3400)
    n = int(np.prod(shape))
    ws = (np.arange(n, dtype=np.uint64) + 1).reshape(shape)
    lab = (np.arange(n, dtype=np.uint64)[::-1] * 3).reshape(shape)
    with _lib.Context(0) as fresh:
        fresh.set_profiling(1)
        got = check(fresh, ws, lab, (2, 2, 1000), None, cap_hint=1)
        assert len(got['counts']) == n == 40800 and (got['counts'] == 1).all() and 2 * n > 1 << 16
        # two C calls (the host arrays hold 1 triple, then n): the pass runs as the rule says
        assert fresh.profile()['k_nl_overlaps']['count'] == table_launches(n, [1, n])
        got = check(fresh, ws, lab.astype(np.uint32), (2, 2, 1000), 0, cap_hint=1)
        assert len(got['counts']) == n - 1


def _node_labels(ctx, ws, lab, n, **kw):
    dw, dl = _dev(ws), _dev_labels(lab)
    got = ctx.node_labels(dw, dl, n, **kw)
    np.testing.assert_array_equal(_host(dw), ws)
    return got


def test_gpu_node_labels_ties_and_absent_nodes(ctx):
    """node 1 is shared exactly in half by labels 9 and 4 (the smaller wins), node 2 is absent from
    the volume, node 3 has one label, node 6 lies beyond number_of_labels"""
    ws = np.zeros((4, 6, 70), dtype=np.uint64)
    lab = np.zeros((4, 6, 70), dtype=np.uint16)
    ws[:2] = 1
    lab[0], lab[1] = 9, 4
    ws[2], lab[2] = 3, 65535
    ws[3], lab[3, :, :40], lab[3, :, 40:] = 6, 8, 2
    for n in (7, 5, 4, 2):
        got = _node_labels(ctx, ws, lab, n, with_counts=True)
        want = NR.max_overlaps(NR.label_overlaps(ws, lab), n, with_counts=True)
        assert got.dtype == np.uint64 and got.shape == (n, 2)
        np.testing.assert_array_equal(got, want)
        labels = _node_labels(ctx, ws, lab, n)
        assert labels.shape == (n,) and labels.dtype == np.uint64
        np.testing.assert_array_equal(labels, want[:, 0])
    got = _node_labels(ctx, ws, lab, 7, with_counts=True)
    assert got.tolist() == [[0, 0], [4, 420], [0, 0], [65535, 420], [0, 0], [0, 0], [8, 240]]
    # with label 4 ignored node 1 goes to 9
    assert _node_labels(ctx, ws, lab, 3, ignore_label=4, with_counts=True).tolist() == [[0, 0], [9, 420], [0, 0]]
    assert _node_labels(ctx, ws, lab, 0).shape == (0,)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint64])
def test_gpu_node_labels_against_restatement(ctx, main_case, dtype):
    """node_labels over the block grid, with and without relabelling (2^64 - 2 as a label), and
    max_overlaps on uploaded triples in any order"""
    from cluster_tools_amd import _lib
    ws, lab8 = main_case
    lab = lab8.astype(dtype)
    lab[lab8 == 255] = _top(dtype)
    for ignore in (None, 0):
        table = NR.label_overlaps(ws, lab, BLOCK, ignore)
        for n in (40, 17, 64):
            want = NR.max_overlaps(table, n, with_counts=True)
            got = _node_labels(ctx, ws, lab, n, block_shape=BLOCK, ignore_label=ignore, with_counts=True)
            np.testing.assert_array_equal(got, want)
            np.testing.assert_array_equal(_lib.max_overlaps_table(table, n, True), want)
        p = np.random.default_rng(5).permutation(len(table['counts']))
        shuffled = {k: v[p] for k, v in table.items()}
        np.testing.assert_array_equal(ctx.max_overlaps(40, shuffled, with_counts=True), NR.max_overlaps(table, 40, True))
    big = {'ws_ids': [2, 2, 2], 'label_ids': [2 ** 64 - 1, 5, 7], 'counts': [2 ** 32 + 1, 2 ** 32 + 1, 2 ** 32]}
    assert ctx.max_overlaps(3, big, with_counts=True).tolist() == [[0, 0], [0, 0], [5, 2 ** 32 + 1]]
    assert ctx.max_overlaps(2, _lib.merge_label_overlaps([]), with_counts=True).tolist() == [[0, 0], [0, 0]]


def test_gpu_node_labels_deterministic(ctx, main_case):
    ws, lab = main_case
    dw, dl = _dev(ws), _dev_labels(lab.astype(np.uint16))
    a = ctx.label_overlaps(dw, dl, block_shape=BLOCK, ignore_label=0)
    na = ctx.node_labels(dw, dl, 40, block_shape=BLOCK, ignore_label=0, with_counts=True)
    b = ctx.label_overlaps(dw, dl, block_shape=BLOCK, ignore_label=0)
    nb = ctx.node_labels(dw, dl, 40, block_shape=BLOCK, ignore_label=0, with_counts=True)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes()
    assert na.tobytes() == nb.tobytes()


def test_gpu_node_labels_arguments(ctx):
    import torch
    ws = _dev(np.ones((2, 3, 4), dtype=np.uint64))
    with pytest.raises(AssertionError):
        ctx.label_overlaps(ws, torch.zeros((2, 3, 4), dtype=torch.float32, device='cuda'))
    with pytest.raises(AssertionError):
        ctx.label_overlaps(ws, torch.zeros((2, 3, 5), dtype=torch.uint8, device='cuda'))
    got = ctx.label_overlaps(ws, torch.full((2, 3, 4), -1, dtype=torch.int8, device='cuda'))       # bits as unsigned
    assert got['label_ids'].tolist() == [255] and got['counts'].tolist() == [24]


def test_gpu_node_labels_integration_block(ctx, main_case):
    """INTEGRATION.md's node-label block, executed as written"""
    from conftest import integration_blocks
    (block,) = [b for b in integration_blocks() if 'def node_labels_on_device' in b]
    ns = {}
    exec(compile(block, 'INTEGRATION.md#node_labels', 'exec'), ns)
    ws, lab = main_case
    table = NR.label_overlaps(ws, lab, BLOCK, 0)
    overlaps, best = ns['node_labels_on_device'](ctx, _dev(ws), _dev_labels(lab), 40, BLOCK, 0)
    NR.assert_overlaps_equal(overlaps, table)
    np.testing.assert_array_equal(best, NR.max_overlaps(table, 40, True))
    pieces = [(_dev(ws[:4, :6]), _dev_labels(lab[:4, :6])), (_dev(ws[4:, :6]), _dev_labels(lab[4:, :6])),
              (_dev(ws[:, 6:]), _dev_labels(lab[:, 6:]))]
    merged, best = ns['node_labels_of_pieces'](ctx, pieces, 40, BLOCK, 0)
    NR.assert_overlaps_equal(merged, table)
    np.testing.assert_array_equal(best, NR.max_overlaps(table, 40, True))
