"""examples/cg_multi.py: four CG solves sharing one multi-vector SpMV per iteration converge on
the SPD example matrix, eagerly and with the iteration captured in a graph; every column is held
to the bound test_gpu_examples.py holds cg.py to."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("graph", [False, True])
def test_cg_multi_example_converges(graph):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "cg_multi.py"), "--grid", "300", "--iters", "150",
           "--nvec", "4"]
    if graph:
        cmd.append("--graph")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    res = [float(part.split()[0]) for part in out.stdout.split("relative residual")[1:]]
    assert len(res) == 4, out.stdout
    assert all(r < 1e-8 for r in res), out.stdout
    assert "native=1" in out.stdout, out.stdout  # the 5-point Laplacian takes the one-pass kernel
