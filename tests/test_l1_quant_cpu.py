"""The l1 fast path's quantiser and bound (nmslib_zig_amd/csrc/l1_quant.hpp) without a GPU."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_l1_quant_header_standalone_under_host_sanitizers(tmp_path):
    """tests/l1_quant_check.cpp includes csrc/l1_quant.hpp alone (no HIP) and checks, for every (query, row) pair of random
    rows, a constant column, values of 1e-30 and 1e30, and queries inside the rows' range, outside it and exactly on lo and
    hi, that |L1 - X_q - s SAD| <= E_q and that the proof's floor stays below the f32 distance; constant data and rows with
    inf or NaN must be declined (checked by the program).  Every byte it produced equals rint((x - lo) / s), clamped, in
    numpy's f64 (checked here)."""
    exe, out = str(tmp_path / "l1_quant_check"), str(tmp_path / "l1.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "l1_quant_check.cpp"), "-o", exe])
    run = subprocess.run([exe, out], capture_output=True, text=True)
    assert run.returncode == 0 and "l1 quant ok" in run.stdout, run.stdout + run.stderr
    assert run.stdout.count("declined") == 4, run.stdout
    raw = open(out, "rb").read()
    off, cases, seen_edges = 0, 0, 0
    while off < len(raw):
        n, dim, nq = (int(v) for v in np.frombuffer(raw, np.uint32, 3, off))
        off += 12
        lo = np.frombuffer(raw, np.float32, dim, off).astype(np.float64)
        off += 4 * dim
        s = float(np.frombuffer(raw, np.float64, 1, off)[0])
        off += 8
        rows = np.frombuffer(raw, np.float32, n * dim, off).reshape(n, dim)
        off += 4 * n * dim
        rb = np.frombuffer(raw, np.uint8, n * dim, off).reshape(n, dim)
        off += n * dim
        q = np.frombuffer(raw, np.float32, nq * dim, off).reshape(nq, dim)
        off += 4 * nq * dim
        qb = np.frombuffer(raw, np.uint8, nq * dim, off).reshape(nq, dim)
        off += nq * dim
        hi = rows.max(0).astype(np.float64)
        np.testing.assert_array_equal(lo, rows.min(0).astype(np.float64))
        assert s == (hi - lo).max() / 255.0
        np.testing.assert_array_equal(rb, np.rint((rows.astype(np.float64) - lo) / s).astype(np.uint8))
        qc = np.clip(q.astype(np.float64), lo, hi)
        np.testing.assert_array_equal(qb, np.rint((qc - lo) / s).astype(np.uint8))
        widest = int(np.argmax(hi - lo))
        assert rb[:, widest].min() == 0 and rb[:, widest].max() == 255       # the widest column spans the byte range
        seen_edges += int((qb[:, widest] == 0).any() and (qb[:, widest] == 255).any())
        cases += 1
    assert off == len(raw) and cases == 6 and seen_edges == 6
