"""numpy restatement of the reference SizeFilterWorkflow's semantics (TEST INFRASTRUCTURE ONLY:
the product path is cc_size_filter in cluster_tools_amd/csrc/cc_size_filter.hip).  It is pinned
bit-exactly to the reference's own jobs by the goldens (test_size_filter_golden.py) and checks
the device at shapes and ids the reference's dense count array cannot take.

  find_uniques.py:105-179        ids, counts = np.unique(labels, return_counts=True)
  size_filter_blocks.py:112      size_threshold: discard ids with count < threshold
  size_filter_blocks.py:116-117  target_number: keep the k ids with the largest counts; the
                                 reference's order among equal counts is an unstable argsort,
                                 fixed here: among equal counts the larger id ranks first (the
                                 reverse of a stable ascending sort by count)
  background_size_filter.py:121-129  discarded ids -> 0
  find_labeling.py:106-116       relabel: the filtered volume's sorted ids get start, start + 1,
                                 ... with start = 0 when 0 occurs in the filtered volume, else 1
"""
import numpy as np


def label_sizes(labels):
    ids, counts = np.unique(np.asarray(labels, dtype=np.uint64), return_counts=True)
    return ids, counts.astype(np.uint64)


def select_discard(ids, counts, size_threshold=None, target_number=None, discard_ids=None):
    """The sorted occurring ids the selection discards."""
    assert sum(x is not None for x in (size_threshold, target_number, discard_ids)) == 1
    if size_threshold is not None:
        return ids[counts < np.uint64(size_threshold)] if size_threshold < 1 << 64 else ids.copy()
    if target_number is not None:
        order = np.argsort(counts, kind='stable')[::-1]        # ids ascending within equal counts, reversed
        return np.sort(ids[order[target_number:]])
    return ids[np.isin(ids, np.asarray(discard_ids, dtype=np.uint64))]


def size_filter(labels, size_threshold=None, target_number=None, discard_ids=None, relabel=True):
    """-> (output volume, dict(ids, counts, discard_ids, assignments, max_id))"""
    labels = np.asarray(labels, dtype=np.uint64)
    ids, counts = label_sizes(labels)
    gone = select_discard(ids, counts, size_threshold, target_number, discard_ids)
    out = labels.copy()
    out[np.isin(labels, gone)] = 0
    uniques = np.unique(out)
    if relabel:
        start = 0 if uniques[0] == 0 else 1
        new_ids = np.arange(start, start + len(uniques), dtype=np.uint64)
        out = new_ids[np.searchsorted(uniques, out)]
    else:
        new_ids = uniques
    assignments = np.stack([uniques, new_ids], axis=1)
    return out, dict(ids=ids, counts=counts, discard_ids=gone, assignments=assignments,
                     max_id=int(new_ids[-1]))
