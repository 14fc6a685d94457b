"""The divergence filter's operands, bound and plan (nmslib_zig_amd/csrc/diverg_filter.hpp) without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_diverg_filter_header_standalone_under_host_sanitizers(tmp_path):
    """tests/diverg_filter_check.cpp includes the header alone (no HIP) and checks, for the five forms at D = 1, 15, 16, 17
    and 256 over random rows, tiny and huge elements, zeros and near-copies of a query, that filter_floor stays at or below
    the f32 distance in DivAcc's order and |key + C_q - d| <= E_q; that a query with a zero, a NaN or an infinity gets no
    proof; and the plan's gates on either side of each edge."""
    exe = str(tmp_path / "diverg_filter_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "diverg_filter_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "diverg filter ok" in run.stdout, run.stdout + run.stderr
    # (Itakura-Saito: the 1e-20 query's reciprocals against the 1e30 rows leave f32's range, so it goes without a proof too)
    assert run.stdout.count("9 of 12 queries with a proof") == 20 and run.stdout.count("is D=") == 5, run.stdout
    assert run.stdout.count("8 of 12 queries with a proof") == 5, run.stdout
