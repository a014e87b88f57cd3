"""examples/pcg.py: CG preconditioned by symmetric Gauss-Seidel (two spmv_hw.TriSolve handles built
from the same full matrix, unknowns in red-black order) reaches the tolerance it was given and
takes fewer iterations than plain CG on the same system, eagerly and with the iteration captured in
a graph.

Grid 64, shift 0.1, tol 1e-8: a scipy restatement on the CPU (same matrix, same recurrences,
convergence looked at every 5 iterations as the example does) takes 75 iterations of plain CG and
40 of the preconditioned one. The test asserts only the inequality."""
import importlib.util
import os

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

GRID, TOL = 64, 1e-8


def _example():
    spec = importlib.util.spec_from_file_location("pcg_example", os.path.join(ROOT, "examples", "pcg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("graph", [False, True])
def test_pcg_example_reaches_its_tolerance_in_fewer_iterations_than_cg(graph, capsys):
    out = _example().main(["--grid", str(GRID), "--tol", str(TOL)] + (["--graph"] if graph else []))
    print(capsys.readouterr().out, out)
    assert out["tol"] == TOL and out["n"] == GRID * GRID
    assert out["levels_red_black"] == 2 and out["levels_natural"] == 2 * GRID - 1
    for name in ("cg", "pcg"):
        assert out[name]["residual"] <= TOL, out
    assert 0 < out["pcg"]["iters"] < out["cg"]["iters"], out
