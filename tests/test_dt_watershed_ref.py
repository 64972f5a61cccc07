"""tests/_dt_watershed_ref.py (the numpy restatement the GPU tests of the distance-transform
watershed compare against) on hand-built cases whose answers are written out here, and the job's
id arithmetic (cluster_tools_amd/watershed/watershed.py: block_ids) on the same cases.  No GPU."""
import numpy as np

import _dt_watershed_ref as R
import _seeds_ref as SR

from _dt_watershed_ref import FIRST_PASS, FILTERED_24, column_slices as _slice, columns as _columns

# The slice of three column seeds (COLUMN_VALUES in _dt_watershed_ref.py, with the reasoning):
# labels 1 1 1 2 2 2 3 3 of sizes 24, 24, 16; size_filter 24 keeps 1 and 2 and hands x = 6, 7 to 2.
assert FIRST_PASS == (1, 1, 1, 2, 2, 2, 3, 3) and FILTERED_24 == (1, 1, 1, 2, 2, 2, 2, 2)


def test_height_map_two_voxels_by_hand():
    # one domain (1, 1, 4): dt = 1 2 3 5 -> dt - min = 0 1 2 4 -> n = 0 .25 .5 1 -> 1 - n = 1 .75 .5 0
    inp = np.array([[[0.5, 0.25, 1.0, 0.0]]], dtype=np.float32)
    dt = np.array([[[1, 2, 3, 5]]], dtype=np.float32)
    h = R.height_map(inp, dt, (1, 1, 4), True, alpha=0.8, sigma_weights=0)
    a, b = np.float32(0.8), np.float32(1.0 - 0.8)          # 1 - .8 in double, then to float32
    assert a.view(np.uint32) == 0x3F4CCCCD and b.view(np.uint32) == 0x3E4CCCCD
    # voxel 0: fl(a * .5) = 0x3ECCCCCD (exact), fl(b * 1) = b; their sum rounds to 0x3F19999A
    assert h[0, 0, 0].view(np.uint32) == 0x3F19999A
    # voxel 1: fl(a * .25) = 0x3E4CCCCD (exact), fl(b * .75) = 0x3E19999A; the sum 0x3EB33334
    assert h[0, 0, 1].view(np.uint32) == 0x3EB33334
    # voxel 3: 1 - n = 0: a * 0 + b * 0
    assert h[0, 0, 3] == 0
    # a domain of constant dt: n = 0, h = a * in + b
    h = R.height_map(inp, np.full((1, 1, 4), 7, dtype=np.float32), (1, 1, 4), True, alpha=0.8, sigma_weights=0)
    assert h[0, 0, 3].view(np.uint32) == 0x3E4CCCCD
    # alpha 1 and 0: the input alone, the inverted distances alone
    np.testing.assert_array_equal(R.height_map(inp, dt, (1, 1, 4), True, 1.0, 0), inp)
    np.testing.assert_array_equal(R.height_map(inp, dt, (1, 1, 4), True, 0.0, 0),
                                  np.array([[[1, .75, .5, 0]]], dtype=np.float32))


def test_three_seeds_without_filter():
    values, seeds = _slice()
    lab, max_ids = R.watershed_domains(values, seeds, [3], (1, 8, 8), True, 0)
    np.testing.assert_array_equal(lab, _columns(FIRST_PASS))
    assert max_ids.tolist() == [3]


def test_filter_keeps_exact_size_and_hands_the_rest_to_the_neighbour():
    values, seeds = _slice()
    lab, max_ids = R.watershed_domains(values, seeds, [3], (1, 8, 8), True, 24)
    np.testing.assert_array_equal(lab, _columns(FILTERED_24))
    assert max_ids.tolist() == [2]


def test_everything_filtered_gives_zeros():
    values, seeds = _slice()
    for size_filter in (25, 65, 10 ** 6):                  # 65: larger than the domain
        lab, max_ids = R.watershed_domains(values, seeds, [3], (1, 8, 8), True, size_filter)
        assert not lab.any() and max_ids.tolist() == [0]


def test_mask_zeroes_the_output_after_the_filter():
    values, seeds = _slice()
    mask = np.ones((1, 8, 8), dtype=np.uint8)
    mask[0, :, 3:] = 0                                     # label 2 is outside the mask entirely
    lab, max_ids = R.watershed_domains(values, seeds, [3], (1, 8, 8), True, 24, mask)
    want = _columns(FILTERED_24)
    want[0, :, 3:] = 0
    np.testing.assert_array_equal(lab, want)               # sizes counted the voxels outside the mask
    assert max_ids.tolist() == [1]


def test_slice_offset_is_the_surviving_maximum_not_the_seed_count():
    from cluster_tools_amd.utils import volume_utils as vu
    from cluster_tools_amd.watershed.watershed import block_ids
    values, seeds = _slice(2)
    lab, max_ids = R.watershed_domains(values, seeds, [3, 3], (2, 8, 8), True, 24)
    assert max_ids.tolist() == [2, 2]
    ids = SR.unique_ids(lab, max_ids, (2, 8, 8), (2, 8, 8), True)
    np.testing.assert_array_equal(ids[0], _columns(FILTERED_24)[0])
    # slice 1 continues after 2, the surviving maximum of slice 0 (the seed count would give 4, 5)
    np.testing.assert_array_equal(ids[1], _columns(FILTERED_24)[0] + np.uint64(2))
    # the job's own arithmetic, in the second of two blocks: + 1 * prod(block_shape)
    big = np.concatenate([np.zeros_like(lab), lab], axis=2)
    blocking = vu.Blocking([0, 0, 0], [2, 8, 16], [2, 8, 8])
    mx = np.array([[0, 2], [0, 2]]).reshape(2, 1, 2)
    obj = np.ones(big.shape, dtype=np.uint8)
    got = block_ids(big, mx, obj, None, blocking, 1, True)
    np.testing.assert_array_equal(got, ids + np.uint64(128))


def test_block_without_voxel_above_threshold_is_the_constant():
    from cluster_tools_amd.utils import volume_utils as vu
    from cluster_tools_amd.watershed.watershed import block_ids
    x = np.zeros((1, 4, 8), dtype=np.float32)
    mask = np.ones(x.shape, dtype=np.uint8)
    mask[0, 0, 5] = 0
    # the input is 1 outside the mask, so with a mask no voxel is above a threshold of 1 or more only
    out, written, stages = R.job(x, (1, 4, 4), mask, threshold=1.0)
    want = np.zeros(x.shape, dtype=np.uint64)
    want[:, :, 4:] = 16
    want[0, 0, 5] = 0
    np.testing.assert_array_equal(out, want)               # block 0: the constant is 0
    unmasked = np.zeros(x.shape, dtype=np.uint64)
    unmasked[:, :, 4:] = 16
    np.testing.assert_array_equal(R.job(x, (1, 4, 4))[0], unmasked)      # the default threshold, no mask
    assert written.all() and stages == {0: None, 1: None}
    blocking = vu.Blocking([0, 0, 0], [1, 4, 8], [1, 4, 4])
    obj = np.zeros(x.shape, dtype=np.uint8)
    for b in (0, 1):
        got = block_ids(np.zeros(x.shape, dtype=np.uint64), np.zeros((1, 1, 2), dtype=np.int64), obj, mask, blocking, b,
                        True)
        np.testing.assert_array_equal(got, want[:, :, 4 * b:4 * b + 4])
    # a block whose mask is empty is not written
    mask[:, :, :4] = 0
    out, written, _ = R.job(x, (1, 4, 4), mask, threshold=1.0)
    assert not written[:, :, :4].any() and written[:, :, 4:].all()
    assert block_ids(np.zeros(x.shape, dtype=np.uint64), np.zeros((1, 1, 2), dtype=np.int64), obj, mask, blocking, 0,
                     True) is None


def test_job_runs_the_chain_per_block():
    # two blocks of (2, 16, 16), slices of blobs: the job's ids are the per-domain labels of the
    # block's own chain with the offsets on the non-zero voxels
    rng = np.random.default_rng(5)
    x = rng.random((2, 16, 32)).astype(np.float32)
    for ax in (1, 2):
        x = (x + np.roll(x, 1, axis=ax) + np.roll(x, -1, axis=ax)) / np.float32(3)
    out, written, stages = R.job(x, (2, 16, 16), sigma_seeds=0.7, sigma_weights=0.7, size_filter=5)
    assert written.all() and out.all()
    for block_id, bb in enumerate(R.blocks(x.shape, (2, 16, 16))):
        lab, max_ids = stages[block_id]
        assert lab.all() and (max_ids >= 1).all()
        want = lab.copy()
        want[1] += np.uint64(max_ids[0])
        np.testing.assert_array_equal(out[bb], want + np.uint64(block_id * 512))
        # every segment that survived holds at least size_filter voxels
        for z in range(2):
            assert np.unique(lab[z], return_counts=True)[1].min() >= 5
