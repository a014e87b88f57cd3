"""CPU-side checks of the transposed-product C-ABI (spmv_*_op, spmv_plan_get_op,
spmv_csr_transpose_device; include/csr_hw_wrapper.h Part 2): the symbols are exported from every
build, declared and listed, and every argument check answers before any HIP call (no GPU here)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import spmv_hw
from conftest import ROOT

NEW = ["spmv_plan_create_device_op", "spmv_plan_create_host_op", "spmv_plan_get_op", "spmv_csr_transpose_device",
       "spmv_multi_create_device_op", "spmv_multi_create_host_op"]


@pytest.mark.parametrize("ablations", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_transpose_symbols_are_exported_declared_and_listed(dtype, ablations):
    path = spmv_hw.lib_path(dtype, ablations)
    assert os.path.exists(path), "run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(NEW) <= exported
    assert set(NEW) <= set(spmv_hw.EXPORTS)
    header = open(os.path.join(ROOT, "include", "csr_hw_wrapper.h")).read()
    assert all(f"int {name}(" in header for name in NEW)
    assert "#define SPMV_OP_N 0" in header and "#define SPMV_OP_T 1" in header
    assert (spmv_hw.OP_N, spmv_hw.OP_T) == (0, 1)
    lib = spmv_hw.load(dtype, ablations)
    assert all(getattr(lib.L, name).argtypes is not None for name in NEW)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bad_op_and_null_arguments_return_codes_without_a_gpu(dtype):
    lib = spmv_hw.load(dtype)
    L = lib.L
    err = lambda: L.spmv_hw_last_error().decode()
    m = lib.make_csr_matrix(np.array([0, 1, 2], np.uint32), np.array([0, 1], np.uint32), np.ones(2, dtype), 2)
    h = ctypes.c_void_p()
    for op in (-1, 2):
        for call in (lambda: L.spmv_plan_create_device_op(ctypes.byref(h), 0, op, 0, 4, 0, None, None, None, None),
                     lambda: L.spmv_plan_create_host_op(ctypes.byref(h), 0, op, ctypes.byref(m), 0, 2),
                     lambda: L.spmv_multi_create_device_op(ctypes.byref(h), 0, op, 0, 4, 0, None, None, None, 2, None),
                     lambda: L.spmv_multi_create_host_op(ctypes.byref(h), 0, op, ctypes.byref(m), 0, 2, 2)):
            assert call() != 0
            assert "op" in err() and "SPMV_OP_T" in err() and not h.value
    T = spmv_hw.OP_T
    # null arguments of the transposed creates, the transpose itself and get_op
    assert L.spmv_plan_create_device_op(None, 0, T, 0, 4, 0, None, None, None, None) != 0
    assert "null argument" in err()
    assert L.spmv_plan_create_device_op(ctypes.byref(h), 0, T, 4, 4, 0, None, None, None, None) != 0
    assert "null argument" in err()
    assert L.spmv_plan_create_host_op(ctypes.byref(h), 0, T, None, 0, 0) != 0
    assert "bad arguments" in err()
    assert L.spmv_plan_create_host_op(ctypes.byref(h), 0, T, ctypes.byref(m), 1, 3) != 0
    assert "bad arguments" in err()
    assert L.spmv_multi_create_device_op(None, 0, T, 0, 4, 0, None, None, None, 2, None) != 0
    assert "null argument" in err()
    assert L.spmv_multi_create_device_op(ctypes.byref(h), 0, T, 4, 4, 0, None, None, None, 2, None) != 0
    assert "null argument" in err()
    assert L.spmv_multi_create_host_op(ctypes.byref(h), 0, T, None, 0, 0, 2) != 0
    assert "bad arguments" in err()
    for nvec in (0, 9):
        assert L.spmv_multi_create_device_op(ctypes.byref(h), 0, T, 0, 4, 0, None, None, None, nvec, None) != 0
        assert "nvec" in err() and not h.value
        assert L.spmv_multi_create_host_op(ctypes.byref(h), 0, T, ctypes.byref(m), 0, 2, nvec) != 0
        assert "nvec" in err() and not h.value
    assert L.spmv_csr_transpose_device(0, 4, 4, 0, None, None, None, 0x1000, None, None, None) != 0
    assert "null argument" in err()
    assert L.spmv_csr_transpose_device(0, 0, 4, 0, None, None, None, None, None, None, None) != 0
    assert "null argument" in err()
    op = ctypes.c_int(7)
    assert L.spmv_plan_get_op(None, ctypes.byref(op)) != 0
    assert "null argument" in err() and op.value == 7


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_op_n_is_the_existing_create_and_reports_its_errors(dtype):
    """op = SPMV_OP_N forwards to the functions without an op: the same codes and messages."""
    lib = spmv_hw.load(dtype)
    L = lib.L
    err = lambda: L.spmv_hw_last_error().decode()
    m = lib.make_csr_matrix(np.array([0, 1, 2], np.uint32), np.array([0, 1], np.uint32), np.ones(2, dtype), 2)
    h = ctypes.c_void_p()
    N = spmv_hw.OP_N
    pairs = [
        (lambda: L.spmv_plan_create_device(None, 0, 4, 4, 0, None, None, None, None),
         lambda: L.spmv_plan_create_device_op(None, 0, N, 4, 4, 0, None, None, None, None)),
        (lambda: L.spmv_plan_create_host(ctypes.byref(h), 0, ctypes.byref(m), 1, 3),
         lambda: L.spmv_plan_create_host_op(ctypes.byref(h), 0, N, ctypes.byref(m), 1, 3)),
        (lambda: L.spmv_multi_create_device(ctypes.byref(h), 0, 0, 4, 0, None, None, None, 9, None),
         lambda: L.spmv_multi_create_device_op(ctypes.byref(h), 0, N, 0, 4, 0, None, None, None, 9, None)),
        (lambda: L.spmv_multi_create_device(ctypes.byref(h), 0, 4, 4, 0, None, None, None, 2, None),
         lambda: L.spmv_multi_create_device_op(ctypes.byref(h), 0, N, 4, 4, 0, None, None, None, 2, None)),
        (lambda: L.spmv_multi_create_host(ctypes.byref(h), 0, ctypes.byref(m), 0, 2, 0),
         lambda: L.spmv_multi_create_host_op(ctypes.byref(h), 0, N, ctypes.byref(m), 0, 2, 0)),
        (lambda: L.spmv_multi_create_host(ctypes.byref(h), 0, None, 0, 0, 2),
         lambda: L.spmv_multi_create_host_op(ctypes.byref(h), 0, N, None, 0, 0, 2)),
    ]
    for old, new in pairs:
        rc_old, msg_old = old(), err()
        rc_new, msg_new = new(), err()
        assert rc_old != 0 and rc_new == rc_old and msg_new == msg_old and msg_old


def test_python_layer_has_the_transpose_keyword_and_entry_points():
    import inspect
    for fn in (spmv_hw.Plan.from_device, spmv_hw.Plan.from_host, spmv_hw.MultiPlan.from_device,
               spmv_hw.MultiPlan.from_host):
        assert inspect.signature(fn).parameters["transpose"].default is False
    assert isinstance(spmv_hw.Plan.op, property)
    assert list(inspect.signature(spmv_hw.csr_transpose).parameters)[:5] == ["lib", "row_ptr", "col", "val", "nr_cols"]
