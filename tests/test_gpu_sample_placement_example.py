"""GPU: examples/sample_placement.py as a user runs it, in a child process: 12 x 11 x 10 sites,
64 samples, 8 sensors; the dense and the factored row list the same picks."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_prints_the_same_picks():
    cmd = [sys.executable, os.path.join(ROOT, "examples", "sample_placement.py"), "--sites", "12",
           "11", "10", "--samples", "64", "--k", "8"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    print(res.stdout)
    print(res.stderr[-2000:])
    assert res.returncode == 0
    lines = res.stdout.splitlines()
    assert "same picks" in lines
    rows = [line for line in lines if line.startswith(("dense", "factored"))]
    assert len(rows) == 2 and rows[0].startswith("dense")
    picks = [line[line.index("["):] for line in rows]
    assert picks[0] == picks[1] and picks[0].count(",") == 7
