"""The short scan's rotation, gate and error bound (nmslib_zig_amd/csrc/short_scan_plan.hpp) without a GPU.

tests/short_scan_plan_check.cpp includes the header alone (no HIP), built with the host sanitizers.  The bound is restated
here in f64: for every (query, row) pair the exact inner product must lie within E_s of the head score the filter would
compute (f32 heads under the stored rotation, fp16 operands, f32 accumulation).  The bound's terms come from
short_scan_plan.hpp's derivation; nothing here is fitted to the data."""
import os
import subprocess

import numpy as np
import pytest

from nmslib_zig_amd.datasets import s_gauss, s_lowrank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("short_scan") / "short_scan_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "short_scan_plan_check.cpp"), "-o", exe])
    return exe


def test_jacobi_is_orthogonal_and_sorted(check_exe):
    run = subprocess.run([check_exe, "jacobi"], capture_output=True, text=True)
    assert run.returncode == 0 and "short scan jacobi ok" in run.stdout, run.stdout + run.stderr


def _bound(check_exe, tmp_path, rows, queries):
    rp, qp, op = (str(tmp_path / n) for n in ("rows.f32", "queries.f32", "out.f64"))
    rows.tofile(rp)
    queries.tofile(qp)
    run = subprocess.run([check_exe, "bound", rp, qp, op, str(len(rows)), str(len(queries))], capture_output=True, text=True)
    assert run.returncode == 0 and "short scan bound written" in run.stdout, run.stdout + run.stderr
    out = np.fromfile(op, dtype=np.float64)
    gate, b_tail, bmax = out[0] != 0, out[1], out[2]
    es = out[4:4 + len(queries)]
    head = out[4 + len(queries):].reshape(len(queries), len(rows))
    exact = queries.astype(np.float64) @ rows.astype(np.float64).T
    return gate, b_tail, bmax, es, np.abs(exact - head)


def test_bound_holds_and_gate_opens_on_lowrank_rows(check_exe, tmp_path):
    rows, queries = s_lowrank(4096, 128, 42), s_lowrank(64, 128, 43)
    gate, b_tail, bmax, es, err = _bound(check_exe, tmp_path, rows, queries)
    print("lowrank: b_tail %.4g bmax %.4g E_s mean %.4g worst error / E_s %.4g" % (b_tail, bmax, es.mean(), (err / es[:, None]).max()))
    assert gate and b_tail <= bmax / 16
    assert (err <= es[:, None]).all()


def test_bound_holds_and_gate_closes_on_gaussian_rows(check_exe, tmp_path):
    rows, queries = s_gauss(4096, 128, 42), s_gauss(64, 128, 43)
    gate, b_tail, bmax, es, err = _bound(check_exe, tmp_path, rows, queries)
    print("gauss: b_tail %.4g bmax %.4g E_s mean %.4g worst error / E_s %.4g" % (b_tail, bmax, es.mean(), (err / es[:, None]).max()))
    assert not gate
    assert (err <= es[:, None]).all()
