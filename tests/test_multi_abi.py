"""CPU-side checks of the multi-vector C-ABI (spmv_multi_*, include/csr_hw_wrapper.h Part 2): the
symbols are exported, the argument checks answer before any HIP call, and the ctypes mirror of
spmv_multi_stats has the C struct's layout."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import spmv_hw
from conftest import ROOT

MULTI = ["spmv_multi_create_device", "spmv_multi_create_host", "spmv_multi_run", "spmv_multi_get_stats",
         "spmv_multi_destroy"]


@pytest.mark.parametrize("ablations", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_multi_symbols_are_exported(dtype, ablations):
    path = spmv_hw.lib_path(dtype, ablations)
    assert os.path.exists(path), "run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(MULTI) <= exported
    assert set(MULTI) <= set(spmv_hw.EXPORTS)
    header = open(os.path.join(ROOT, "include", "csr_hw_wrapper.h")).read()
    assert all(f"{name}(" in header for name in MULTI)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_multi_argument_errors_return_codes_without_a_gpu(dtype):
    """A bad nvec, a null handle and a misaligned X / Y return nonzero with a message, and none of
    them reaches a HIP call (this test runs with no GPU). Without a GPU no handle exists, so the
    misalignment seen here is the one that holds for every nvec: a pointer that is no multiple of
    sizeof(ValueType). The per-nvec rule, min(16, nvec * sizeof(ValueType)), is checked on the
    GPU (tests/test_gpu_multi.py)."""
    lib = spmv_hw.load(dtype)
    L = lib.L
    err = lambda: L.spmv_hw_last_error().decode()
    h = ctypes.c_void_p()
    for nvec in (0, 9, -1):
        assert L.spmv_multi_create_device(ctypes.byref(h), 0, 0, 4, 0, None, None, None, nvec, None) != 0
        assert "nvec" in err() and not h.value
    assert L.spmv_multi_create_device(None, 0, 0, 4, 0, None, None, None, 2, None) != 0
    assert "null argument" in err()
    assert L.spmv_multi_create_device(ctypes.byref(h), 0, 4, 4, 0, None, None, None, 2, None) != 0
    assert "null argument" in err()
    m = lib.make_csr_matrix(np.array([0, 1, 2], np.uint32), np.array([0, 1], np.uint32), np.ones(2, dtype), 2)
    for nvec in (0, 9):
        assert L.spmv_multi_create_host(ctypes.byref(h), 0, ctypes.byref(m), 0, 2, nvec) != 0
        assert "nvec" in err() and not h.value
    assert L.spmv_multi_create_host(ctypes.byref(h), 0, ctypes.byref(m), 1, 3, 2) != 0
    assert "bad arguments" in err()
    assert L.spmv_multi_create_host(ctypes.byref(h), 0, None, 0, 0, 2) != 0
    assert "bad arguments" in err()
    # run: null handle; X or Y off by half a value
    assert L.spmv_multi_run(None, 0x10000, 0x20000, None) != 0
    assert "null handle" in err()
    half = np.dtype(dtype).itemsize // 2
    assert L.spmv_multi_run(None, 0x10000 + half, 0x20000, None) != 0
    assert "misaligned" in err()
    assert L.spmv_multi_run(None, 0x10000, 0x20000 + half, None) != 0
    assert "misaligned" in err()
    st = spmv_hw.spmv_multi_stats()
    assert L.spmv_multi_get_stats(None, ctypes.byref(st)) != 0
    assert "null argument" in err()
    L.spmv_multi_destroy(None)  # a no-op, like free(NULL)


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "csr_hw_wrapper.h"
#define F(f) printf(#f " %zu\n", offsetof(spmv_multi_stats, f))
int main(void) {
    printf("sizeof %zu\n", sizeof(spmv_multi_stats));
    F(nr_rows); F(nr_cols); F(nr_nzeros); F(device_bytes); F(algorithmic_bytes);
    F(device); F(nvec); F(native); F(kernel); F(format);
    return 0;
}
"""


@pytest.mark.parametrize("double", [1, 0])
def test_multi_stats_ctypes_mirror_matches_the_c_struct(tmp_path, double):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-DDOUBLE={double}", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = dict(ln.split() for ln in out.splitlines())
    S = spmv_hw.spmv_multi_stats
    assert int(got.pop("sizeof")) == ctypes.sizeof(S)
    assert [name for name, _ in S._fields_] == list(got)  # same fields, same order
    for name, _ in S._fields_:
        assert int(got[name]) == getattr(S, name).offset, name
