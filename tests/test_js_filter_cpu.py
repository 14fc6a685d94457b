"""The Jensen-Shannon filter's constants, bound and plan (nmslib_zig_amd/csrc/diverg_js_filter.hpp) without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_js_filter_header_standalone_under_host_sanitizers(tmp_path):
    """tests/js_filter_check.cpp includes the header alone (no HIP) and checks, at D = 1, 5, 100 and 257 over random
    histograms with zeros on either side, tiny elements and elements above 1, that |key + C_q - v| <= E_q and floor <= v
    for the key of a software model of the loop with the logarithm at either end of its ulp range; that a NaN, infinite or
    negative query element gives no proof; the square-root floor; and the plan's gates."""
    exe = str(tmp_path / "js_filter_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "js_filter_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "js filter ok" in run.stdout, run.stdout + run.stderr
    assert run.stdout.count("9 of 12 queries with a proof") == 4, run.stdout
