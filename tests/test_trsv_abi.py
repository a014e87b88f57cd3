"""CPU-side checks of the triangular solve's C-ABI (include/csr_hw_wrapper.h Part 5): every
spmv_trsv_* symbol is exported by both precisions of both builds, the stats struct has the header's
layout, and bad arguments come back as return codes with a message before any HIP call. No GPU."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import spmv_hw

TRSV_SYMBOLS = ["spmv_trsv_create_device", "spmv_trsv_create_host", "spmv_trsv_solve", "spmv_trsv_get_stats",
                "spmv_trsv_destroy"]


@pytest.mark.parametrize("ablations", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_trsv_symbols_are_exported(dtype, ablations):
    import os
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "csr_hw_wrapper.h")).read()
    declared = sorted(set(re.findall(r"\b(spmv_trsv_[a-z_]+)\s*\(", header)))
    assert declared == sorted(TRSV_SYMBOLS)
    assert set(TRSV_SYMBOLS) <= set(spmv_hw.EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", spmv_hw.lib_path(dtype, ablations)], check=True,
                         capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not set(TRSV_SYMBOLS) - exported


def test_trsv_stats_struct_and_constants_match_the_header():
    assert ctypes.sizeof(spmv_hw.spmv_trsv_stats) == 7 * 8 + 4 * 4
    assert [f for f, _ in spmv_hw.spmv_trsv_stats._fields_] == [
        "n", "nr_nzeros", "nr_levels", "nr_launches", "nr_chain_levels", "max_level_rows", "device_bytes",
        "device", "uplo", "diag", "reserved"]
    assert (spmv_hw.TRSV_LOWER, spmv_hw.TRSV_UPPER, spmv_hw.TRSV_DIAG_NONUNIT, spmv_hw.TRSV_DIAG_UNIT) == (0, 1, 0, 1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_trsv_argument_errors_return_codes_without_a_gpu(dtype):
    lib = spmv_hw.load(dtype)
    L = lib.L
    h = ctypes.c_void_p()
    m = lib.make_csr_matrix(np.array([0, 1, 2], np.uint32), np.array([0, 1], np.uint32), np.ones(2), 2)
    rect = lib.make_csr_matrix(np.array([0, 1, 2], np.uint32), np.array([0, 1], np.uint32), np.ones(2), 3)
    st = spmv_hw.spmv_trsv_stats()
    one = ctypes.c_void_p(8)  # a non-null address no call may reach
    cases = [
        (lambda: L.spmv_trsv_create_device(ctypes.byref(h), 0, 2, 0, 4, 0, one, None, None, None), "uplo must be"),
        (lambda: L.spmv_trsv_create_device(ctypes.byref(h), 0, -1, 0, 4, 0, one, None, None, None), "uplo must be"),
        (lambda: L.spmv_trsv_create_device(ctypes.byref(h), 0, 0, 2, 4, 0, one, None, None, None), "diag must be"),
        (lambda: L.spmv_trsv_create_device(None, 0, 0, 0, 4, 0, one, None, None, None), "null argument"),
        (lambda: L.spmv_trsv_create_device(ctypes.byref(h), 0, 0, 0, 4, 0, None, None, None, None), "null argument"),
        (lambda: L.spmv_trsv_create_host(ctypes.byref(h), 0, 5, 0, ctypes.byref(m)), "uplo must be"),
        (lambda: L.spmv_trsv_create_host(ctypes.byref(h), 0, 1, 7, ctypes.byref(m)), "diag must be"),
        (lambda: L.spmv_trsv_create_host(None, 0, 0, 0, ctypes.byref(m)), "bad arguments"),
        (lambda: L.spmv_trsv_create_host(ctypes.byref(h), 0, 0, 0, None), "bad arguments"),
        (lambda: L.spmv_trsv_create_host(ctypes.byref(h), 0, 0, 0, ctypes.byref(rect)), "must be square"),
        (lambda: L.spmv_trsv_solve(None, one, one, None), "null handle"),
        (lambda: L.spmv_trsv_get_stats(None, ctypes.byref(st)), "null argument"),
    ]
    for call, msg in cases:
        assert call() != 0
        assert msg in L.spmv_hw_last_error().decode(), (msg, L.spmv_hw_last_error().decode())
    assert not h.value
    L.spmv_trsv_destroy(None)  # a null handle is ignored, as free() ignores it


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_empty_handle_needs_no_gpu(dtype):
    """n == 0: create makes an empty handle without touching a device, its solve enqueues nothing
    (null vectors are fine), its stats are zero; a null b or x with n > 0 is refused per call on a
    real handle (GPU suite)."""
    lib = spmv_hw.load(dtype)
    L = lib.L
    for make in (lambda h: L.spmv_trsv_create_device(ctypes.byref(h), 0, 1, 1, 0, 0, None, None, None, None),
                 lambda h: L.spmv_trsv_create_host(ctypes.byref(h), 0, 0, 0, ctypes.byref(
                     lib.make_csr_matrix(np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0), 0)))):
        h = ctypes.c_void_p()
        assert make(h) == 0, L.spmv_hw_last_error().decode()
        assert h.value
        assert L.spmv_trsv_solve(h, None, None, None) == 0
        st = spmv_hw.spmv_trsv_stats()
        assert L.spmv_trsv_get_stats(h, ctypes.byref(st)) == 0
        assert (st.n, st.nr_nzeros, st.nr_levels, st.nr_launches, st.device_bytes) == (0, 0, 0, 0, 0)
        assert L.spmv_trsv_get_stats(h, None) != 0
        L.spmv_trsv_destroy(h)
