"""bench.py without --full: the headline workload alone, set up, warmed up, timed and reported; the other workloads run
only to write what --dump-outputs writes for them, and the legs that check or compare (recall, CPU baseline,
host-pointer entry) run only under --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("hnsw", "sift", "cos768x")
DUMPED = sorted(f"{w}_{a}.npy" for w in ("bruteforce",) + OTHERS for a in ("ids", "distances", "counts"))


def _bench(args, tmp_path):
    env = dict(os.environ)
    for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "NMSLIB_GPU_DEVICE", "NMSLIB_GPU_SHARDS", "BENCH_BACKEND"):
        env.pop(v, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), r.stderr


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone(tmp_path):
    common = ["--gpus", "1", "--n", "200000", "--rows-per-gpu", "20000", "--steps", "2", "--warmup", "1"]
    plain, log = _bench(common, tmp_path)
    assert plain["n_gpus"] == 1 and plain["steps"] == 2 and plain["config"]["rows"] == 200000
    assert plain["metric"].startswith("queries/sec @ recall@10") and plain["unit"] == "queries/s"
    assert plain["higher_is_better"] is True and plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["dtype"]
    for key in ("workloads", "recall_at_k", "cpu_baseline", "host_entry", "value_host_entry"):
        assert key not in plain, key
    for w in OTHERS:
        assert f"[{w}]" not in log, f"a plain run without --dump-outputs ran {w}"

    dumped, _ = _bench(common + ["--dump-outputs", str(tmp_path / "plain")], tmp_path)
    assert "workloads" not in dumped and "recall_at_k" not in dumped
    assert sorted(os.listdir(tmp_path / "plain")) == DUMPED

    full, _ = _bench(common + ["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")], tmp_path)
    assert full["recall_at_k"] == 1.0 and full["distances_match_reference"] is True and "host_entry" in full
    assert sorted(full["workloads"]) == sorted(OTHERS)
    assert full["metric"] == plain["metric"] and full["dtype"] == plain["dtype"]
    assert sorted(os.listdir(tmp_path / "full")) == DUMPED
    for f in DUMPED:                     # the same timed paths, the same answers
        np.testing.assert_array_equal(np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f), err_msg=f)


def test_ef_sweep_needs_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "hnsw", "--ef-sweep", "64"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 2 and "--ef-sweep needs --full" in r.stderr, r.stderr[-2000:]
