import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ham_fast_plan_header_standalone_under_host_sanitizers(tmp_path):
    """tests/ham_fast_plan_check.cpp includes csrc/ham_fast_plan.hpp alone (no HIP): served / not served at the gate's
    edges; for n of 65 536 to 5 000 000 the splits cover every row once, none is longer than 65 536 rows, nsplit * k <= 8192"""
    exe = str(tmp_path / "ham_fast_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "ham_fast_plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "ham fast plan ok" in run.stdout, run.stdout + run.stderr
