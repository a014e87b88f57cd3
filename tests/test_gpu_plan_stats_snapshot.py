"""What a plan reports about its layout, pinned: for every golden matrix, every forced
SPMV_HW_KERNEL name and both precisions, the layout fields of stats() and the drop-in wrapper's
hw_matrix sizes (one unit) equal tests/golden/plan_stats_snapshot.json, recorded once by
tools/record_plan_stats.py from the library as it stood before the per-kernel dispatch moved into
the layout table. The test never rewrites the snapshot. y of one run is checked too:
test_gpu_parity's tolerances, gold / fpga / fp64 slices bitwise as there.
"""
import json
import os
import sys

import pytest

import oracle
import spmv_hw
from conftest import DTYPES, FIXTURES, GOLDEN, ROOT, golden_arrays, manifest
from test_gpu_parity import _bitwise, check

sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_plan_stats as rec  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def snapshot():
    with open(os.path.join(GOLDEN, "plan_stats_snapshot.json")) as f:
        return json.load(f)


def test_snapshot_covers_every_case(snapshot):
    assert sorted(snapshot) == sorted(rec.key(tag, name, k) for _, tag in DTYPES for name in FIXTURES
                                      for k in rec.KERNELS)
    for e in snapshot.values():
        assert "error" in e or (sorted(e["stats"]) == sorted(rec.STATS_FIELDS)
                                and sorted(e["hw_matrix"]) == sorted(rec.HW_FIELDS))


@pytest.mark.parametrize("kernel", rec.KERNELS)
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("dtype,tag", DTYPES)
def test_plan_stats_match_snapshot(snapshot, monkeypatch, dtype, tag, name, kernel):
    import torch
    assert torch.cuda.is_available()
    for k, v in rec.env_of(kernel).items():
        monkeypatch.setenv(k, v)
    lib = spmv_hw.load(dtype)
    _, c, row_ptr, col, val, _ = oracle.read_csr(os.path.join(GOLDEN, manifest()[name]["file"]), dtype)
    x, y_gold = golden_arrays(name, tag)
    want = snapshot[rec.key(tag, name, kernel)]
    got, y = rec.entry(torch, lib, kernel, row_ptr, col, val, x, c)
    assert got == want
    if "error" in want:  # the create failed when the snapshot was recorded, with this text
        pytest.skip("create fails on this pair, as recorded: " + want["error"])
    assert got["stats"]["kernel"] == rec.KERNELS.index(kernel)
    check(row_ptr, col, val, x, y_gold, y, dtype)
    if kernel == "gold" or (kernel == "slices" and tag == "f64"):
        _bitwise(y, y_gold)
    if kernel in ("fpga", "blocked"):  # the defaults: VF = 1, 32768-column blocks
        _bitwise(y, oracle.spmv_fpga_order(row_ptr, col, val, x, c, 32768, 1))
