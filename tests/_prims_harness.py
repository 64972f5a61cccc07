"""ctypes binding of the test-only harness library of the device primitives
(tests/prims_harness, built by __graft_entry__.build())."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, 'tests', 'prims_harness', 'libprims_harness.so')
CONSTANTS = ('SC_TILE', 'SC_SINGLE_MAX', 'RS_TILE', 'SU_T', 'SU_MAX')

_lib = None


def load():
    """The harness library with its entries' signatures set; fails the test if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(HARNESS):
        pytest.fail('tests/prims_harness/libprims_harness.so not built (__graft_entry__.build())')
    import torch  # noqa: F401  (one HIP runtime per process, torch's: see cluster_tools_amd._lib.load)
    L = ctypes.CDLL(HARNESS)
    P, I, N = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    L.ph_last_error.restype = ctypes.c_char_p
    L.ph_last_error.argtypes = []
    L.ph_constants.argtypes = [ctypes.POINTER(N)]
    L.ph_scan_u32.argtypes = L.ph_scan_u64.argtypes = [P, P, N]
    L.ph_sort_keys_u64.argtypes = [P, P, N, I, I]
    L.ph_sort_pairs_u64_u32.argtypes = L.ph_sort_pairs_u64_u64.argtypes = [P, P, P, P, N, I, I]
    L.ph_select_unique_u64.argtypes = [P, P, P, N]
    L.ph_select_flagged_u64.argtypes = [P, P, P, P, N]
    L.ph_pairs_sort_unique_small.argtypes = [P, P, N, I, P, N, P, P, P]
    L.ph_seam_map_small.argtypes = [P, N, P, P, P]
    _lib = L
    return L


def constants():
    """SC_TILE, SC_SINGLE_MAX, RS_TILE, SU_T, SU_MAX of the harness's copy of cc_prims.hip, by name."""
    out = (ctypes.c_int64 * len(CONSTANTS))()
    assert load().ph_constants(out) == 0
    return dict(zip(CONSTANTS, (int(v) for v in out)))


def ok(rc):
    """Assert that an entry returned 0, with its message otherwise."""
    assert rc == 0, 'harness entry failed: %s' % load().ph_last_error().decode()
