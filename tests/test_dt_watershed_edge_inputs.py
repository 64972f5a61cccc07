"""tests/_dt_watershed_edge_inputs.py (the inputs of tests/test_gpu_dt_watershed_edges.py) pinned on the
CPU: where each builder puts its extrema, run ends, empty domains and seeds, and what
tests/_dt_watershed_ref.py makes of them on cases whose answers are worked out by hand.  No GPU."""
import numpy as np

import _dt_watershed_edge_inputs as E
import _dt_watershed_ref as R


def test_extremum_cases_hold_one_minimum_and_one_maximum_in_different_rows():
    for apply_2d in (True, False):
        dom = E.extremum_domain(apply_2d)
        assert dom in list(R.blocks(E.EXT_SHAPE, R.domain_shape(E.EXT_BS, apply_2d)))
        for x in E.EXT_X:
            for last_row in (False, True):
                for last_slice in ((False,) if apply_2d else (False, True)):
                    inp, dt, at_min, at_max = E.extremum_case(apply_2d, x, last_row, last_slice)
                    assert dt[at_min] == 0 and dt[at_max] == 50 and (dt == 0).sum() == 1 and (dt == 50).sum() == 1
                    assert dt.min() == 0 and dt.max() == 50 and np.partition(dt.ravel(), 1)[1] >= 1
                    inside = np.zeros(dt.shape, dtype=bool)
                    inside[dom] = True
                    assert inside[at_min] and inside[at_max]
                    assert at_min[2] == at_max[2] == 300 + x and {at_min[1], at_max[1]} == {0, 23}
                    assert at_min[1] == (23 if last_row else 0)
                    if not apply_2d:
                        assert at_min[0] == int(last_slice) and at_max[0] == 1 - int(last_slice)
    # the two extrema decide every voxel of the domain and nothing outside it
    inp, dt, at_min, at_max = E.extremum_case(True, 256, False)
    want = R.height_map(inp, dt, E.EXT_BS, True, 0.8, 0)
    for at in (at_min, at_max):
        mid = dt.copy()
        mid[at] = E.EXT_MID
        differs = R.height_map(inp, mid, E.EXT_BS, True, 0.8, 0).view(np.uint32) != want.view(np.uint32)
        assert differs[E.extremum_domain(True)].sum() > 24 * 300 // 2 and differs.sum() == differs[E.extremum_domain(True)].sum()


def test_band_slices_layout():
    values, seeds = E.band_slices()
    assert values.shape == seeds.shape == (1, 3, 600) and seeds.all()
    assert (values == values[:, :1]).all() and len(np.unique(values[0, 0])) == 600 and (np.diff(values[0, 0]) > 0).all()
    row = seeds[0, 0].tolist()
    assert (seeds == seeds[:, :1]).all()
    # the band edges: lanes 62 | 63, 63 | 0 (twice) and 0 | 1 of a wave; runs across x = 256 and x = 512
    heads = [0] + [x for x in range(1, 600) if row[x] != row[x - 1]]
    assert heads == [0, 63, 64, 128, 193, 320, 449] and [h % 64 for h in heads] == [0, 63, 0, 0, 1, 0, 1]
    assert row[255] == row[256] == 6 and row[511] == row[512] == 2 and row[63] == 2
    ids, sizes = np.unique(seeds[0, 0], return_counts=True)
    assert dict(zip(ids.tolist(), sizes.tolist())) == {3: 63, 5: 64, 1: 65, 6: 127, 4: 129, 2: 152}
    assert sorted(sizes.tolist()) == list(E.BAND_SIZES)


def test_band_filter_by_hand():
    values, seeds = E.band_slices()
    bs = (1, 3, 600)
    lab, max_ids = R.watershed_domains(values, seeds, [6], bs, True, 0)
    np.testing.assert_array_equal(lab, seeds)
    # 192 = 3 * 64: id 3 (3 * 63 voxels) goes to the 2 at x = 63; id 5 holds exactly 192 and stays
    lab, max_ids = R.watershed_domains(values, seeds, [6], bs, True, 192)
    np.testing.assert_array_equal(lab, np.tile(E.band_row(E.BANDS_FILTERED_192), (1, 3, 1)))
    assert max_ids.tolist() == [6]
    # 193: id 5 goes too: to the 2 on its left, its last column (reached at its own cost from both) to 1
    lab, max_ids = R.watershed_domains(values, seeds, [6], bs, True, 193)
    want = np.tile(E.band_row(E.BANDS_FILTERED_193), (1, 3, 1))
    assert want[0, 0, 126] == 2 and want[0, 0, 127] == 1
    np.testing.assert_array_equal(lab, want)
    assert max_ids.tolist() == [6]
    # the two bands of id 2 count together: 3 * 152 stays, one more and only nothing is left
    lab, max_ids = R.watershed_domains(values, seeds, [6], bs, True, 456)
    assert (lab == 2).all() and max_ids.tolist() == [2]
    lab, max_ids = R.watershed_domains(values, seeds, [6], bs, True, 457)
    assert not lab.any() and max_ids.tolist() == [0]
    # every filter of the GPU test decides another outcome
    kept = [len(np.unique(R.watershed_domains(values, seeds, [6], bs, True, 3 * w + e)[0]))
            for w in E.BAND_SIZES for e in (0, 1)]
    assert kept == [6, 5, 5, 4, 4, 3, 3, 2, 2, 1, 1, 1]        # the last: only the label 0


def test_band_volume_has_an_empty_domain_between_seeded_ones():
    values, seeds, counts = E.band_volume()
    doms = list(R.blocks(E.BAND_VOLUME_SHAPE, E.BAND_VOLUME_BS))
    assert len(doms) == 6 and counts.tolist() == [6, 0, 6, 7, 0, 6]
    for d, bb in enumerate(doms):
        assert seeds[bb].any() == (counts[d] > 0) and int(seeds[bb].max()) <= counts[d]
        assert seeds[bb].all() or not seeds[bb].any()
    assert doms[1] == np.s_[0:1, 0:3, 600:1200]
    lab, max_ids = R.watershed_domains(values, seeds, counts, E.BAND_VOLUME_BS, True, 193)
    np.testing.assert_array_equal(lab[doms[0]], np.tile(E.band_row(E.BANDS_FILTERED_193), (1, 3, 1)))
    np.testing.assert_array_equal(lab[doms[3]], lab[doms[0]])
    assert max_ids.tolist() == [6, 0, 6, 6, 0, 6] and not lab[doms[1]].any() and not lab[doms[4]].any()
    assert not np.array_equal(lab[doms[2]], lab[doms[0]])
    # the last domain: the same sizes per id, the one-column band at lane 62 with the next head at lane 63
    row = seeds[doms[5]][0, 0].tolist()
    assert [x for x in range(1, 600) if row[x] != row[x - 1]] == [63, 190, 191, 255, 320, 449] and row[190] == 2
    ids, sizes = np.unique(seeds[doms[5]][0, 0], return_counts=True)
    assert dict(zip(ids.tolist(), sizes.tolist())) == {3: 63, 5: 64, 1: 65, 6: 127, 4: 129, 2: 152}


def test_flat_and_slice_cases():
    for shape, bs in (((4, 17, 36), (2, 5, 7)), ((1, 1, 1), (1, 1, 1)), ((5, 1, 1), (5, 1, 1)), ((1, 1, 300), (1, 1, 300))):
        values, seeds, counts = E.flat_case(shape, bs)
        assert len(np.unique(values)) == (5 if values.size > 100 else len(np.unique(values)))
        assert seeds.flat[0] == 1 and seeds.flat[-1] != 0
        doms = list(R.blocks(shape, R.domain_shape(bs, True)))
        assert len(doms) == len(counts)
        for d, bb in enumerate(doms):                       # 1 .. n_d, each once
            s = seeds[bb]
            assert sorted(s[s != 0].tolist()) == list(range(1, int(counts[d]) + 1))
    values, seeds, counts = E.first_slice_case()
    assert counts[0] > 10 and counts[1:].tolist() == [0, 0] and not seeds[1:].any()
    lab, max_ids = R.watershed_domains(values, seeds, counts, values.shape, True)
    assert lab[0].all() and not lab[1:].any() and max_ids.tolist() == [int(counts[0]), 0, 0]


def test_unseeded_domain_case():
    values, seeds, counts = E.unseeded_domain_case()
    assert counts.reshape(2, 3, 3)[:, 1, 1].tolist() == [0, 0] and (np.delete(counts, [4, 13]) > 0).all()
    assert not seeds[E.UNSEEDED_CENTRE].any()
    for border in (np.s_[:, 32, 65:130], np.s_[:, 66, 65:130], np.s_[:, 33:66, 64], np.s_[:, 33:66, 130]):
        assert seeds[border].all()
    lab, max_ids = R.watershed_domains(values, seeds, counts, E.UNSEEDED_BS, True)
    assert not lab[E.UNSEEDED_CENTRE].any() and (lab != 0).sum() == lab.size - 2 * 33 * 65
    assert max_ids.reshape(2, 3, 3)[:, 1, 1].tolist() == [0, 0]


def test_tiled_prenormalized_keeps_the_zero_corridor():
    import _watershed_ref as WR
    for apply_2d in (True, False):
        x, seeds, counts, shape = E.tiled_prenormalized(apply_2d)
        assert shape == (6, 40, 80) and shape[1] > 32 and shape[2] > 64           # two flat tiles on both axes
        assert counts.tolist() == [49] * (6 if apply_2d else 1)
        for v in WR.PRENORMALIZED_VALUES:
            assert (np.isnan(x).any() if v != v else (x.view(np.uint32) == np.float32(v).view(np.uint32)).any())
        lab, _ = R.watershed_domains(x, seeds, counts, shape, apply_2d)
        assert lab[WR.ZERO_CORRIDOR].tolist() == [5, 5, 5, 2, 2]                  # -0.0 lies below +0.0
        equal_zeros = np.where(x == 0, np.float32(0), x)
        lab, _ = R.watershed_domains(equal_zeros, seeds, counts, shape, apply_2d)
        assert lab[WR.ZERO_CORRIDOR].tolist() == [5, 2, 2, 2, 2]
