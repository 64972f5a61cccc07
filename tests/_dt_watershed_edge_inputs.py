"""Inputs of tests/test_gpu_dt_watershed_edges.py (TEST INFRASTRUCTURE ONLY): volumes that put the
edges of cc_watershed_height_map's and cc_watershed_domains' kernels where a wrong kernel shows --
a domain's only minimum and maximum in a chosen wave and stride, bands of seed ids whose runs end at
chosen lanes, domains around the flat tile's extent, values taken as they are.  The reference they
are run through is tests/_dt_watershed_ref.py; tests/test_dt_watershed_edge_inputs.py pins them on
hand-worked cases.

Keep every domain at or below the 50 000 voxels _watershed_ref.block allows."""
import functools

import numpy as np

import _watershed_ref as WR
from _dt_watershed_ref import blocks, number_seeds


# The height map's statistics (k_wd_stats: 256 threads stride over a row segment, wave shuffles,
# LDS atomics, global atomics).  2-D domains of 24 x 300 and 2 x 300, 3-D ones of 2 x 24 x 300
# clipped to 1 x 2 x 300: a row segment of 300 takes a second stride of 44 voxels.
EXT_SHAPE, EXT_BS = (3, 26, 600), (2, 24, 300)
EXT_X = (0, 63, 64, 255, 256, 299)              # lane 0, the last lane, wave 1, the last thread, the second stride
EXT_MID = 15.0


def extremum_domain(apply_2d):
    """the chosen domain: the second x-domain of the first y-domain, in 2-D of slice 1"""
    return np.s_[1:2, 0:24, 300:600] if apply_2d else np.s_[0:2, 0:24, 300:600]


@functools.lru_cache(maxsize=None)
def _extremum_base():
    rng = np.random.default_rng(11)
    inp = rng.random(EXT_SHAPE).astype(np.float32)
    dt = rng.uniform(1, 30, EXT_SHAPE).astype(np.float32)
    for a in (inp, dt):
        a.setflags(write=False)
    return inp, dt


def extremum_case(apply_2d, x, last_row, last_slice=False):
    """(inp, dt, at_min, at_max): dt random in [1, 30] but for one voxel of 0 and one of 50 in the
    chosen domain, both at in-domain column x: the minimum in the domain's first (last_row: last)
    row, the maximum in the other one; of a 3-D domain the minimum in its first (last_slice: last)
    slice and the maximum in the other one."""
    inp, dt = _extremum_base()
    dt = dt.copy()
    dom = extremum_domain(apply_2d)
    z = (dom[0].start, dom[0].stop - 1)
    y = (dom[1].start, dom[1].stop - 1)
    assert apply_2d or z[0] != z[1]
    at_min = (z[bool(last_slice)], y[bool(last_row)], dom[2].start + x)
    at_max = (z[not last_slice], y[not last_row], dom[2].start + x)
    dt[at_min], dt[at_max] = 0, 50
    return inp, dt, at_min, at_max


# The size filter's histogram (k_wd_hist: runs of equal labels in a wave add once, from their first
# lane).  Every voxel is a seed; the ids are bands along x:
#   width   63     1     64      65       127       129       151
#   x       0-62   63    64-127  128-192  193-319   320-448   449-599
#   id      3      2     5       1        6         4         2
# so runs end between lanes 62 | 63, 63 | 0 (x = 64, 128) and 0 | 1 (x = 193), and cross x = 256 and
# x = 512; id 2 holds two bands, 152 columns.  The value of column x is x / 1024: it rises along x,
# so a removed band between the regions L (left) and R is reached from L at the cost of the voxel
# itself and from R at the cost of the band's last column -- L takes it, but for that last column,
# which both reach at the same cost: min(L, R).  A removed band at the left edge goes to R.
BAND_WIDTHS = (63, 1, 64, 65, 127, 129, 151)
BAND_IDS = (3, 2, 5, 1, 6, 4, 2)
BAND_ROWS = 3
BAND_SIZES = (63, 64, 65, 127, 129, 152)        # columns per id, in ascending order: ids 3, 5, 1, 6, 4, 2
# size_filter 3 * 64 over 3 rows: id 3 (189 voxels) goes to id 2 at x = 63, id 5 (exactly 192) stays
BANDS_FILTERED_192 = ((64, 2), (64, 5), (65, 1), (127, 6), (129, 4), (151, 2))
# size_filter 193: id 5 goes as well: x = 64 .. 126 to the 2 on its left, x = 127 to min(2, 1)
BANDS_FILTERED_193 = ((127, 2), (66, 1), (127, 6), (129, 4), (151, 2))


# The same bands in another order: the one-column band of id 2 at x = 190, lane 62, a run head in the
# upper half of a wave with the next head (x = 191) in the same wave.  The sizes per id are the same.
BAND_SHUFFLED = ((63, 127, 1, 64, 65, 129, 151), (3, 6, 2, 5, 1, 4, 2))


def band_row(bands):
    """((width, id), ...) -> one row of ids"""
    return np.concatenate([np.full(w, i, dtype=np.uint64) for w, i in bands])


def band_slices(widths=BAND_WIDTHS, rows=BAND_ROWS, ids=BAND_IDS):
    """(values, seeds) of one (1, rows, sum(widths)) domain of such bands"""
    assert len(widths) == len(ids) and len(set(ids)) == len(ids) - 1, 'one id in two bands'
    n = int(sum(widths))
    assert n <= 1024
    values = np.tile((np.arange(n) / np.float32(1024)).astype(np.float32), (1, rows, 1))
    seeds = np.tile(band_row(zip(widths, ids)), (1, rows, 1))
    return values, seeds


BAND_VOLUME_SHAPE, BAND_VOLUME_BS = (1, 9, 1200), (1, BAND_ROWS, 600)
BAND_VOLUME_COUNTS = (6, 0, 6, 7, 0, 6)


def band_volume():
    """(values, seeds, counts): 3 x 2 domains of (1, 3, 600) in raster order: the bands; nothing
    (count 0, no seed, at raster index 1 between two seeded domains); the ids rotated by one band;
    the bands with a count one above the largest id; nothing; BAND_SHUFFLED."""
    values = np.zeros(BAND_VOLUME_SHAPE, dtype=np.float32)
    seeds = np.zeros(BAND_VOLUME_SHAPE, dtype=np.uint64)
    layouts = [(BAND_WIDTHS, BAND_IDS), None, (BAND_WIDTHS, BAND_IDS[1:] + BAND_IDS[:1]), (BAND_WIDTHS, BAND_IDS), None,
               BAND_SHUFFLED]
    for bb, layout in zip(blocks(BAND_VOLUME_SHAPE, BAND_VOLUME_BS), layouts):
        values[bb] = band_slices()[0]
        if layout is not None:
            seeds[bb] = band_slices(layout[0], BAND_ROWS, layout[1])[1]
    return values, seeds, np.asarray(BAND_VOLUME_COUNTS, dtype=np.int64)


def flat_case(shape, block_shape, apply_2d=True):
    """(values, seeds, counts): WR.plateau_field's five levels, its seeds (and the volume's first
    and last voxel) as single-voxel seeds renumbered per domain"""
    full = tuple(max(s, f) for s, f in zip(shape, (17, 33, 66)))
    values, s = WR.plateau_field(shape, full=full)
    picks = s != 0
    picks.flat[0] = picks.flat[-1] = True
    seeds, counts = number_seeds(picks, block_shape, apply_2d)
    return values, seeds, counts


def first_slice_case(shape=(3, 40, 70)):
    """one block of three slices with seeds in slice 0 only: counts [n, 0, 0]"""
    values, s = WR.plateau_field(shape, full=shape)
    picks = s != 0
    picks[1:] = False
    seeds, counts = number_seeds(picks, shape, True)
    return values, seeds, counts


UNSEEDED_SHAPE, UNSEEDED_BS = (2, 99, 195), (2, 33, 65)
UNSEEDED_CENTRE = np.s_[:, 33:66, 65:130]


def unseeded_domain_case():
    """3 x 3 slice domains per slice, the centre one without a seed and every voxel next to it
    across its four borders a seed"""
    values, s = WR.plateau_field(UNSEEDED_SHAPE, full=UNSEEDED_SHAPE)
    picks = s != 0
    picks[UNSEEDED_CENTRE] = False
    picks[:, 32, 65:130] = picks[:, 66, 65:130] = True
    picks[:, 33:66, 64] = picks[:, 33:66, 130] = True
    seeds, counts = number_seeds(picks, UNSEEDED_BS, True)
    return values, seeds, counts


PRENORMALIZED_TILES = (1, 4, 4)                  # (6, 40, 80): two flat tiles of 32 x 64 on both axes


def tiled_prenormalized(apply_2d):
    """(values, seeds, counts, shape): WR.prenormalized_field repeated over y and x, one block; the
    seed ids are its own (1 .. 49, several voxels apart sharing one), every count the largest"""
    x, seeds = WR.prenormalized_field()
    x, seeds = np.tile(x, PRENORMALIZED_TILES), np.tile(seeds, PRENORMALIZED_TILES)
    nd = x.shape[0] if apply_2d else 1
    return x, seeds, np.full(nd, int(seeds.max()), dtype=np.int64), x.shape
