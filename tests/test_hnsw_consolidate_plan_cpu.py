"""The host arithmetic of nmslib_gpu_consolidate (nmslib_zig_amd/csrc/hnsw_consolidate_plan.hpp) without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hnsw_consolidate_plan_header_standalone_under_host_sanitizers(tmp_path):
    """tests/hnsw_consolidate_plan_check.cpp includes csrc/hnsw_consolidate_plan.hpp alone (no HIP, nothing of the engine).
    For n in {1, 31, 33, 65, 70, 1007} it checks, against a row-by-row restatement: the new positions with the rows at the
    word edges 0 / 31 / 32 / 63 / 64 / n - 1 deleted, none, all, a bitset shorter than the rows and random shares; levels,
    up_off and the list of upper-level nodes when nodes move past removed upper-level nodes; the entry point when it is
    deleted, alone and with one or all of the other nodes of the top level (ties go to the smallest position), and that a
    live one stays."""
    exe = str(tmp_path / "hnsw_consolidate_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hnsw_consolidate_plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "hnsw consolidate plan ok" in run.stdout, run.stdout + run.stderr
    # per n: 5 fixed cases + 4 random shares, + 3 for n > 40 (three sizes), + the explicit case
    assert f"{6 * 9 + 3 * 3 + 1} cases" in run.stdout, run.stdout
