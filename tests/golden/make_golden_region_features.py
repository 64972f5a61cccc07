#!/opt/conda/bin/python3.9
"""Generate the region-features golden by running the REFERENCE's own merge function.

Run only in the build container (it needs /root/reference and the conda python):

    /opt/conda/bin/python3.9 tests/golden/make_golden_region_features.py

What runs: the reference's `_extract_and_merge_region_features` (cluster_tools/features/
merge_region_features.py:116-165, with its `merge_feats`), unmodified, imported from
/root/reference with the stand-ins of tests/golden/stubs for the absent dependencies.  It is given

  * the nifty `blocking` stub over the volume,
  * a small in-memory object with `chunks` and `read_chunk` in place of the z5py varlen dataset,
    whose chunks are serialized exactly as region_features.py:181-187 writes them (per block
    float32 [id, count, mean] of the block's ids, nothing for a block of ignore label only,
    region_features.py:152-155),
  * a numpy array as the output dataset.

Only the vigra call (region_features.py:176-177) is stood in for: per block and id the count and
the float64 mean of the normalized input (the reference's vu.normalize(x, 0, 255) for uint8,
(x, 0, 1) for float32: float32 per voxel), all zero for the ignore label as vigra's ignoreLabel
leaves it.  This pins the table layout, the zero rows and the reference's float32 block merging.

Output: tests/golden/region_features_merge.npz (labels, values_u8, values_f32, block_shape,
number_of_labels, node_chunk, table_u8, table_f32), written with fixed zip timestamps, so a rerun
reproduces it byte for byte.
"""
import io
import os
import sys
import types
import zipfile
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
sys.path.insert(0, os.path.join(HERE, 'stubs'))


def _bare_package(name, path):
    mod = types.ModuleType(name)
    mod.__path__ = [path]
    sys.modules[name] = mod
    return mod


# bypass the eager package __init__ imports
_bare_package('cluster_tools', os.path.join(REF, 'cluster_tools'))
_bare_package('cluster_tools.utils', os.path.join(REF, 'cluster_tools', 'utils'))
_bare_package('cluster_tools.features', os.path.join(REF, 'cluster_tools', 'features'))

import nifty.tools as nt  # noqa: E402  (the stub)
import cluster_tools.utils.volume_utils as ref_vu  # noqa: E402
from cluster_tools.features import merge_region_features as ref_merge  # noqa: E402

FEATURE_NAMES = ['count', 'mean']
IGNORE_LABEL = 0


class BlockFeats:
    """the varlen dataset region_features.py writes, in memory"""

    def __init__(self, chunks):
        self.chunks = tuple(chunks)
        self.data = {}

    def write_chunk(self, chunk_id, data, varlen):
        assert varlen
        self.data[tuple(chunk_id)] = data

    def read_chunk(self, chunk_id):
        return self.data.get(tuple(chunk_id))


def block_features(labels, values, block_shape):
    """region_features.py:140-192 with numpy in place of vigra.analysis.extractRegionFeatures"""
    blocking = nt.blocking([0, 0, 0], list(labels.shape), list(block_shape))
    ds_out = BlockFeats(block_shape)
    max_val = 255. if values.dtype == np.dtype('uint8') else 1.
    for block_id in range(blocking.numberOfBlocks):
        block = blocking.getBlock(block_id)
        bb = tuple(slice(b, e) for b, e in zip(block.begin, block.end))
        lab = labels[bb]
        if np.sum(lab != IGNORE_LABEL) == 0:
            continue
        input_ = ref_vu.normalize(values[bb], 0, max_val)
        assert input_.dtype == np.float32
        ids = np.unique(lab)
        # one float32 row [id, count, mean] per id of the block, rows concatenated: the layout
        # region_features.py:181-187 serializes
        rows = np.zeros((len(ids), 1 + len(FEATURE_NAMES)), dtype=np.float32)
        rows[:, 0] = ids
        for k, i in enumerate(ids):
            if i != IGNORE_LABEL:
                x = input_[lab == i].astype(np.float64)
                rows[k, 1:] = (len(x), x.mean())
        ds_out.write_chunk([b // s for b, s in zip(block.begin, block_shape)], rows.reshape(-1), True)
    return blocking, ds_out


def reference_table(labels, values, block_shape, number_of_labels, node_chunk):
    blocking, ds_in = block_features(labels, values, block_shape)
    ds = np.full((number_of_labels, len(FEATURE_NAMES)), -1, dtype=np.float32)
    with redirect_stdout(io.StringIO()):                # the function logs to stdout
        for node_begin in range(0, number_of_labels, node_chunk):
            ref_merge._extract_and_merge_region_features(blocking, ds_in, ds, node_begin,
                                                         min(node_begin + node_chunk, number_of_labels), FEATURE_NAMES)
    return ds


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (reruns are byte-identical)"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            zi = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue())


def main():
    rng = np.random.default_rng(31)
    shape, block_shape = (20, 36, 48), (8, 16, 32)
    labels = np.repeat(rng.integers(0, 60, size=(20, 36, 8)), 6, axis=2).astype(np.uint32)
    labels[labels >= 40] += 15                          # ids 0..39 and 55..74
    labels[:8, :16, :32] = 0                            # a block of ignore label only
    number_of_labels = int(labels.max()) + 4
    values_u8 = rng.integers(0, 256, size=shape, dtype=np.uint8)
    values_f32 = (rng.integers(0, 256, size=shape) / 256.).astype(np.float32)
    node_chunk = 32
    arrays = dict(labels=labels, values_u8=values_u8, values_f32=values_f32,
                  block_shape=np.array(block_shape, dtype=np.int64),
                  number_of_labels=np.array(number_of_labels, dtype=np.int64),
                  node_chunk=np.array(node_chunk, dtype=np.int64),
                  table_u8=reference_table(labels, values_u8, block_shape, number_of_labels, node_chunk),
                  table_f32=reference_table(labels, values_f32, block_shape, number_of_labels, node_chunk))
    for k in ('table_u8', 'table_f32'):
        assert arrays[k].shape == (number_of_labels, 2) and arrays[k].dtype == np.float32
        assert not (arrays[k] == -1).any() and not arrays[k][0].any()
    path = os.path.join(HERE, 'region_features_merge.npz')
    save_npz(path, arrays)
    print(path, os.path.getsize(path), 'bytes;', number_of_labels, 'labels')


if __name__ == '__main__':
    main()
