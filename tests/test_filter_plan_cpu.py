"""The routing rule of a filtered HNSW batch (nmslib_zig_amd/csrc/filter_plan.hpp) without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_filter_plan_header_standalone_under_host_sanitizers(tmp_path):
    """tests/filter_plan_check.cpp includes csrc/filter_plan.hpp alone (no HIP, nothing of the engine).  For ef > k, ef < k
    and ef = k it checks the route at m = 0, 1, k', k' + 1, scan_rows, scan_rows + 1, 4096 and 4097, with scan_rows unset,
    below k', above it and at the capacity; that a k' beyond 4096 does not lift the capacity; the LDS bytes of the scan at
    the edges of its power-of-two key array; and that a scan whose keys and query exceed 160 KB of LDS goes to the walk."""
    exe = str(tmp_path / "filter_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "filter_plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "filter plan ok" in run.stdout, run.stdout + run.stderr
    assert f"{3 * 16 + 4 + 8 + 6} cases" in run.stdout, run.stdout
