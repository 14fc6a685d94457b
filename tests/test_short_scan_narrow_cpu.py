"""The narrow tier of the short scan (a head of 32 rotated columns; nmslib_zig_amd/csrc/short_scan_plan.hpp) without a GPU.

tests/short_scan_narrow_check.cpp includes the header alone (no HIP), is built with the host sanitizers and run directly.
It asserts that head_constants() at 64 columns returns make_rotation()'s constants bit for bit, and restates heads, tails
and E_s at width 32 (the prefix of the stored rotation).  Here, in f64: for every (query, row) pair the exact inner product
lies within E_s of the fp16 head product the filter would compute.  Nothing is fitted to the data."""
import os
import subprocess

import numpy as np
import pytest

from nmslib_zig_amd.datasets import s_lowrank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("short_scan_narrow") / "short_scan_narrow_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "short_scan_narrow_check.cpp"), "-o", exe])
    return exe


def test_narrow_bound_holds_on_lowrank_rows(check_exe, tmp_path):
    rows, queries = s_lowrank(4096, 128, 42), s_lowrank(256, 128, 43)
    rp, qp, op = (str(tmp_path / n) for n in ("rows.f32", "queries.f32", "out.f64"))
    rows.tofile(rp)
    queries.tofile(qp)
    run = subprocess.run([check_exe, rp, qp, op, str(len(rows)), str(len(queries))], capture_output=True, text=True)
    assert run.returncode == 0 and "narrow bound written" in run.stdout, run.stdout + run.stderr
    out = np.fromfile(op, dtype=np.float64)
    gate, b_tail, bmax = out[0] != 0, out[1], out[2]
    es = out[4:4 + len(queries)]
    head = out[4 + len(queries):].reshape(len(queries), len(rows))
    err = np.abs(queries.astype(np.float64) @ rows.astype(np.float64).T - head)
    print("narrow: b_tail %.4g bmax %.4g E_s mean %.4g worst error / E_s %.4g" % (b_tail, bmax, es.mean(), (err / es[:, None]).max()))
    assert gate and b_tail <= bmax / 16
    assert (err <= es[:, None]).all()
