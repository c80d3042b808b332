"""Launcher of tests/_smallnet_child.py, shared by tests/test_smallnet_forms_gpu.py and
tests/test_smallnet_act_gpu.py.  A plain helper module.

The library reads TDE_SN_MFMA once per process, so masks 0 and 7 run in one fresh child process per
(suite, mask).  A child of either suite that ends by signal or at its time limit may have left the GPU in a
bad state: ``guard`` then fails every later GPU test of both files without starting anything."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
CHILD_TIMEOUT = 120     # s: a cold import of torch, loading the code objects, four small plans and their CPU
#                         oracles (about 3 s warm)
TAG = "SMALLNET_CHILD "

_CRASHED = []           # set when a child ends by signal or at its time limit: no GPU work after that
_CHILDREN = {}


def guard():
    if _CRASHED:
        pytest.fail(f"not run: {_CRASHED[0]}")


def run(suite, mask):
    """The child's output for (suite, mask): dict(suite, mask, figs).  Each pair is started at most once."""
    if (suite, mask) in _CHILDREN:
        return _CHILDREN[suite, mask]
    guard()
    env = dict(os.environ, PYTHONPATH=str(REPO), TDE_SN_MFMA=mask)
    try:
        p = subprocess.run([sys.executable, str(REPO / "tests" / "_smallnet_child.py"), suite], env=env,
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=str(REPO))
    except subprocess.TimeoutExpired as e:
        _CRASHED.append(f"the {suite} TDE_SN_MFMA={mask} child hit its {CHILD_TIMEOUT} s limit")
        pytest.fail(f"{_CRASHED[0]}\n{e.stdout}\n{e.stderr}")
    if p.returncode < 0:
        _CRASHED.append(f"the {suite} TDE_SN_MFMA={mask} child ended by signal {-p.returncode}")
        pytest.fail(f"{_CRASHED[0]}\n{p.stdout}\n{p.stderr}")
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [l for l in p.stdout.splitlines() if l.startswith(TAG)]
    assert len(lines) == 1, p.stdout + p.stderr
    out = json.loads(lines[0][len(TAG):])
    assert out["mask"] == mask and out["suite"] == suite
    _CHILDREN[suite, mask] = out
    return out
