"""bench.py's derived fields on the CPU: `value_e2e` (2 nnz / (SpMV step +
the exchange that completes y), the reference's "Total time" = hardware + accumulation,
csr_hw_wrapper.cpp:276-285) and the parser of the reference's timing lines that the `dropin`
field reads from the drop-in child (csr_hw_wrapper.cpp:274,284-285, main.cpp:72)."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
bench = pytest.importorskip("bench")


def _out(**kw):
    d = {"value": 400.0, "n_ranks": 8, "dist_rehearsal": False, "exchange": None}
    d.update(kw)
    return d


def test_value_e2e_one_gpu_is_the_value():
    v, form = bench.value_e2e(_out(n_ranks=1), 0.8, 160e6)
    assert v == 400.0 and "no exchange" in form["form"]


def test_value_e2e_prefers_the_library_reduce():
    ex = {"reduce_ms": 0.5, "native": {"reduce_exchange_ms": 0.2}}
    v, form = bench.value_e2e(_out(exchange=ex), 0.12, 160e6)
    assert v == pytest.approx(2 * 160e6 / (0.32e-3) / 1e9, rel=1e-3)
    assert form["exchange_ms"] == 0.2 and "library RCCL reduce" in form["exchange_src"]
    assert "with_gather" not in form
    ex["native"]["gather_exchange_ms"] = 0.05
    v2, form = bench.value_e2e(_out(exchange=ex), 0.12, 160e6)
    assert v2 == v and form["with_gather"]["value"] == pytest.approx(2 * 160e6 / (0.17e-3) / 1e9, rel=1e-3)


def test_value_e2e_falls_back_to_torch_reduce_then_to_none():
    v, form = bench.value_e2e(_out(exchange={"reduce_ms": 0.5, "native": {"error": "no RCCL"}}), 0.5, 160e6)
    assert v == pytest.approx(320.0) and "torch.distributed" in form["exchange_src"]
    v, form = bench.value_e2e(_out(exchange={"error": "boom"}), 0.5, 160e6)
    assert v is None and form["form"] == "no exchange was measured"
    v, _ = bench.value_e2e(_out(n_ranks=1, dist_rehearsal=True, exchange={"native": {"reduce_exchange_ms": 0.1}}),
                           0.4, 160e6)
    assert v == pytest.approx(640.0)


def test_reference_line_parser():
    text = ("Total non-zeros : 16. Total 1 MB transferred ( in : 0.5, out : 0.5)\n"
            "Matrix read time        : 122.253000 ms elapsed\n"
            "Hardware execution time : 0.873000 ms elapsed\n"
            "Result accumulation time : 1.854000 ms elapsed\n"
            "Total time  : 2.727000 ms elapsed\n"
            "Verification PASSED!\n"
            "Hardware execution time : 0.851000 ms elapsed\n"
            "Hardware execution time : garbled\n")
    assert bench._ref_lines(text, "Hardware execution time") == [0.873, 0.851]
    assert bench._ref_lines(text, "Matrix read time") == [122.253]
    assert bench._ref_lines(text, "Total time") == [2.727]
    assert bench._ref_lines(text, "Software execution time") == []


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs: a y within the budget is written whole in its own precision; a larger one
    as the same seeded sample of rows on every call, with the rows beside it; N ranks share the
    budget and write one file each."""
    import numpy as np
    import torch

    assert bench.DUMP_BUDGET_BYTES + 16 * 1024 <= 64_000_000  # 64 MB in all, 16 .npy headers included
    y = torch.arange(1000, dtype=torch.float32) * 0.5
    bench.dump_outputs(str(tmp_path / "a"), y, 0, 1)
    assert sorted(os.listdir(tmp_path / "a")) == ["y.npy"]
    got = np.load(tmp_path / "a" / "y.npy", allow_pickle=False)
    assert got.dtype == np.float32 and np.array_equal(got, y.numpy())

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2400)
    y64 = y.double()
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), y64, 0, 1)
    rows = np.load(tmp_path / "b" / "y_rows.npy", allow_pickle=False)
    vals = np.load(tmp_path / "b" / "y.npy", allow_pickle=False)
    assert rows.dtype == np.float64 and vals.dtype == np.float64 and len(rows) == len(vals) == 150
    assert rows.nbytes + vals.nbytes <= 2400
    r = rows.astype(np.int64)
    assert np.all(np.diff(r) > 0) and r[0] >= 0 and r[-1] < 1000 and np.array_equal(vals, y64.numpy()[r])
    for f in ("y.npy", "y_rows.npy"):
        assert (tmp_path / "b" / f).read_bytes() == (tmp_path / "c" / f).read_bytes()

    bench.dump_outputs(str(tmp_path / "d"), y64, 1, 2)  # rank 1 of 2: half the budget
    assert sorted(os.listdir(tmp_path / "d")) == ["y_rank1.npy", "y_rows_rank1.npy"]
    assert len(np.load(tmp_path / "d" / "y_rank1.npy", allow_pickle=False)) == 75


def test_plain_and_full_options_parse():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dropin_child_is_in_the_package():
    """The drop-in run is the package's own script (no oracle import: it takes the software y
    from the bench)."""
    path = os.path.join(ROOT, "spmv-fpga_amd", "dropin_main.py")
    src = open(path).read()
    assert "import oracle" not in src and "allow_pickle=False" in src
