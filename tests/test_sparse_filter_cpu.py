"""The sparse inverted-file filter's bounds and plan (nmslib_zig_amd/csrc/sparse_filter.hpp) without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sparse_filter_header_standalone_under_host_sanitizers(tmp_path):
    """tests/sparse_filter_check.cpp includes the header alone (no HIP) and checks, for the four served kinds over random,
    cancelling, one-term, longest-row, tiny-norm and huge rows, that |A - real| <= E_q with A in the kernel's order and that
    the floor stays at or below the f32 distance in the scan's union order; that zero-norm, tiny, non-finite and huge queries
    get no proof; and the plan's gates on either side of each edge."""
    exe = str(tmp_path / "sparse_filter_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "sparse_filter_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "sparse filter ok" in run.stdout, run.stdout + run.stderr
    assert run.stdout.count("16 of 21 queries with a proof") == 4, run.stdout
