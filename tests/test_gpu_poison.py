"""NMSLIB_GPU_POISON: every workspace the engine allocates is filled with a byte before its first use.  The work of
tests/poison_child.py -- one batch per chain through the host ABI and through the device entry, range queries, the HNSW
visited-set variants -- must give the same bits whatever the workspaces held: no kernel reads a word that no kernel wrote."""
import os
import subprocess
import sys

import numpy as np
import pytest

from . import poison_child

pytestmark = pytest.mark.gpu

# Wall time of one child, measured once on an MI355X: 13.0 s (torch import, data generation, four 65536-row indexes and
# two host-built HNSW graphs included).  The time limit is five times that.
CHILD_SECONDS = 13.0
CHILD_TIMEOUT = 5 * CHILD_SECONDS


@pytest.fixture(scope="module")
def plain():
    assert "NMSLIB_GPU_POISON" not in os.environ, "this process must run without the poison fill"
    return poison_child.run_all()


# 255: NaN floats, -1 ints.  127: 3.39e38 floats, 2139062143 ints.
@pytest.mark.parametrize("byte", [255, 127])
def test_poisoned_workspaces_give_the_same_bits(plain, tmp_path, byte):
    out = tmp_path / f"poison_{byte}.npz"
    env = dict(os.environ, NMSLIB_GPU_POISON=str(byte))
    # (one attempt: a non-zero exit, a death by signal or the time limit fails the test)
    r = subprocess.run([sys.executable, poison_child.__file__, str(out)], env=env, timeout=CHILD_TIMEOUT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"child exit {r.returncode}\n{r.stdout[-4000:]}"
    with np.load(out) as z:
        got = {name: z[name] for name in z.files}
    assert sorted(got) == sorted(plain)
    differ = [name for name in sorted(plain) if not np.array_equal(got[name], plain[name])]
    assert not differ, differ
