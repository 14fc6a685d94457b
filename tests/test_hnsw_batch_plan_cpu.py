"""The GPU HNSW builder's batch plan (nmslib_zig_amd/csrc/hnsw_batch_plan.hpp) without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hnsw_batch_plan_header_standalone_under_host_sanitizers(tmp_path):
    """tests/hnsw_batch_plan_check.cpp includes csrc/hnsw_batch_plan.hpp alone (no HIP, nothing of the engine) and drives it as
    the builder's batch loop does.  Level streams: a fixed-seed geometric draw, all zero, strictly increasing, one tall node
    in the middle; n in {1, 2, 17, 1000}, batch_div in {1, 16}, max_batch in {1, 7, 4096}, forward and reverse.  It asserts
    that the batches tile [first, n) with non-empty batches of at most max_batch; that a batch ends at the first position
    above the running top level and never spans the cut; that pts is level-major from the top down with every node at levels
    0 .. min(level, top), src naming the same node one level up (-1 at its highest slice) and the slices covering pts; the
    reverse order; that for every `first` the run started there, with the top level and entry point the pass over
    everything (cut = first) had there, gives the pass's batch ends, pts, src, base and promotions from there on, and (forward)
    a build of the first `first` rows alone gives the pass's batches before the cut; and that assign_up_offsets over [0, n)
    equals [0, n0) followed by [n0, n) for every n0."""
    exe = str(tmp_path / "hnsw_batch_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hnsw_batch_plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "hnsw batch plan ok" in run.stdout, run.stdout + run.stderr
    # 4 streams x 2 orders x 6 size rules, every first in [1, n) of n = 2, 17, 1000
    assert f"{4 * 2 * 6 * (1 + 16 + 999)} cuts" in run.stdout, run.stdout
