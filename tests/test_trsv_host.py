"""The triangular solve's host planner (spmv-fpga_amd/csrc/trsv_plan.cpp) under
-fsanitize=address,undefined: tests/trsv_host builds plan_trsv and build_trsv_layout into a program
of its own and drives them on small matrices, each as a LOWER and as an UPPER problem. No GPU."""
import fcntl
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "tests", "trsv_host")


def test_trsv_planner_host_program_under_sanitizers():
    """n = 0 and 1, a diagonal matrix, a bidiagonal chain (n levels, one chain launch), a 5-point grid
    in natural order (2g - 1 levels of widths 1..g..1) and in red-black order (2 levels), a random
    lower triangle, an arrow matrix, level widths cut - 1, cut, cut + 1, 1, cut + 1 around
    kTrsvChainRows (chain, wide, chain, wide), row lengths at and past the long-row cut in a narrow
    and a wide level, unsorted columns with duplicates, a missing diagonal (its row named under
    NONUNIT, accepted under UNIT) and a column past n. Checked: the levels against a fixed-point
    recomputation, every dependency in a strictly lower level, perm a permutation sorted by
    (level, row), the launch list covering every level once and in order with every maximal narrow
    run merged, the short and long lists partitioning each level, the layout entry for entry, and
    a host substitution over the layout solving the triangle."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    os.makedirs(os.path.join(HOST, "build"), exist_ok=True)
    with open(os.path.join(HOST, "build", ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.run(["make", "-s", "-C", HOST], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([os.path.join(HOST, "build", "trsv_check")], capture_output=True, text=True, timeout=300,
                       env=env)
    assert not [k for k in ("AddressSanitizer", "LeakSanitizer", "runtime error") if k in p.stderr], p.stderr[-4000:]
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("OK trsv plan")
