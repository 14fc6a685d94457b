#!/usr/bin/env python3
"""Compare the GPU HNSW builder of this build with another build of the library (the parent commit's): the bytes of the
graphs it makes and the time it takes (not part of bench.py).

Bytes: each library builds the configurations of CONFIGS with gpu_build=1 and saves the index (save_data=False); the record
holds the sha256 of every file, and of the answers of one 64-query batch where a configuration asks for it.  Every hash
must be equal between the two libraries.

Time: l2, 1M x 128 (s_lowrank of nmslib_zig_amd/datasets.py), M=16, efConstruction=200, gpu_build=1, gpu_append=1: the
engine's build_seconds of the build, and the wall time of the finalize after 10 000 more rows were added.  Legs in the order
parent / new / parent / new / parent; the spread of either figure is max - min of the three parent legs, and the mean of the
new legs must not lie above the mean of the parent legs by more than that.

Every leg is one fresh child process under its own time limit; after a failed leg nothing more is started on the device.

    python3 tools/hnsw_build_compare.py --parent-lib <libnmslib_c.so> [--out profiles/hnsw_builder_refactor_parent_vs_new.json]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, space, rows, dim, index parameters (gpu_build=1 is added); rows: s_gauss(rows, dim, seed), uint8 for l2sqr_sift
CONFIGS = [
    ("l2_M8_efC40", "l2", 3000, 32, dict(M=8, efConstruction=40)),
    ("cosine_M16_post2", "cosinesimil", 3000, 48, dict(M=16, post=2)),
    ("l2_M16_post1", "l2", 3000, 32, dict(M=16, post=1)),
    ("sift_M8", "l2sqr_sift", 2000, 128, dict(M=8)),
    ("l2_M100_delaunay1", "l2", 2000, 16, dict(M=100, delaunay_type=1)),
    ("l2_M4_batch1", "l2", 300, 8, dict(M=4, gpu_build_batch=1)),
]
APPEND_ROWS, APPEND_ADD, APPEND_DIM = 2000, 1000, 32


def log(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def sha_file(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def make(nz, space, X, **params):
    u8 = space == "l2sqr_sift"
    idx = nz.Index(space, "hnsw", data_type="DenseUInt8Vector" if u8 else "DenseVector", dist_type="Int" if u8 else "Float")
    (idx.addUInt8Batch if u8 else idx.addDenseBatch)(X)
    idx.buildIndex(gpu_build=1, **params)
    return idx


def child_bytes():
    import numpy as np

    import nmslib_zig_amd as nz
    from nmslib_zig_amd.datasets import s_gauss
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        def saved(idx, name):
            assert idx.graphBuilder() == 2, f"{name}: not built on the GPU"
            path = os.path.join(tmp, name)
            idx.save(path, save_data=False)
            out[name] = sha_file(path)
            log(f"{name}: {out[name][:16]}")

        for seed, (name, space, n, dim, params) in enumerate(CONFIGS):
            X = s_gauss(n, dim, 700 + seed)
            if space == "l2sqr_sift":
                X = np.clip(np.rint(X * 32 + 128), 0, 255).astype(np.uint8)
            idx = make(nz, space, X, **params)
            saved(idx, name)
            idx.close()
        # duplicate rows, efConstruction above the LDS-table range, M near the cap: the second search attempt's case
        base = np.random.default_rng(5).standard_normal((300, 16)).astype(np.float32)
        idx = make(nz, "l2", np.concatenate([base, base[:200], base[:100]]), M=30, efConstruction=400)
        saved(idx, "l2_duplicates_M30_efC400")
        idx.close()
        # rows added after the build, into the resident graph; with the fp16 copy, and one batch over it
        X, Q = s_gauss(APPEND_ROWS + APPEND_ADD, APPEND_DIM, 710), s_gauss(64, APPEND_DIM, 711)
        for name, extra in (("l2_append", {}), ("l2_append_f16", dict(gpu_rows="f16"))):
            idx = make(nz, "l2", X[:APPEND_ROWS], M=8, efConstruction=60, gpu_append=1, **extra)
            idx.addDenseBatch(X[APPEND_ROWS:], np.arange(APPEND_ROWS, len(X), dtype=np.int32))
            idx.finalize()
            assert int(idx.stats()["rows_appended"]) == APPEND_ADD, f"{name}: the rows were not appended"
            saved(idx, name)
            if extra:
                ids, ds, cnt = idx.knnQueryBatch(Q, 10)
                assert int(idx.stats()["last_path"]) == 5, f"{name}: the batch did not walk the fp16 copy"
                out[name + "_knn64"] = hashlib.sha256(ids.tobytes() + ds.tobytes() + cnt.tobytes()).hexdigest()
            idx.close()
    return out


def child_time(nrows, nadd):
    import numpy as np

    import nmslib_zig_amd as nz
    from nmslib_zig_amd.datasets import s_lowrank
    X = s_lowrank(nrows + nadd, 128, 42)
    idx = nz.Index("l2", "hnsw")
    idx.addDenseBatch(X[:nrows])
    idx.buildIndex(M=16, efConstruction=200, gpu_build=1, gpu_append=1)
    first = idx.stats()
    idx.addDenseBatch(X[nrows:], np.arange(nrows, nrows + nadd, dtype=np.int32))
    t0 = time.perf_counter()
    idx.finalize()
    wall = time.perf_counter() - t0
    st = idx.stats()
    rec = {"rows": nrows, "added": nadd, "build_seconds": first["build_seconds"], "append_finalize_wall_seconds": wall,
           "append_build_seconds": st["build_seconds"], "rows_appended": int(st["rows_appended"]),
           "graph_builder": idx.graphBuilder()}
    idx.close()
    log(f"build {rec['build_seconds']:.3f} s, finalize after the add {wall * 1e3:.1f} ms")
    return rec


def gate(legs, key):
    par = [g[key] for g in legs if g["leg"] == "parent"]
    new = [g[key] for g in legs if g["leg"] == "new"]
    spread, pm, nm = max(par) - min(par), sum(par) / len(par), sum(new) / len(new)
    return {"parent": par, "new": new, "parent_mean": pm, "new_mean": nm, "parent_spread": spread, "ratio": nm / pm,
            "within_spread": bool(nm <= pm + spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libnmslib_c.so of the parent commit, run beside this build")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--add", type=int, default=10_000)
    ap.add_argument("--timeout", type=int, default=150, help="seconds, per leg")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=("bytes", "time"), default=None)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.child:
        if a.lib:
            import nmslib_zig_amd as nz
            nz.LIB_PATH = os.path.abspath(a.lib)   # another build of the library (the parent commit's)
        print(json.dumps(child_bytes() if a.child == "bytes" else child_time(a.rows, a.add)))
        return
    out = {"tool": "tools/hnsw_build_compare.py", "date": time.strftime("%Y-%m-%d"),
           "method": "hashes: sha256 of the index files saved with save_data=False (and of ids, distances and counts of one "
                     "64-query batch); build_seconds: the engine's own clock over the GPU build of the first rows; "
                     "append_finalize_wall_seconds: perf_counter around the finalize after the add; legs in the order run, one "
                     "process each; parent_spread: max - min of the parent legs",
           "hashes": {}, "time_legs": []}

    def leg(tag, kind):
        cmd = [sys.executable, os.path.abspath(__file__), "--parent-lib", a.parent_lib, "--child", kind, "--rows", str(a.rows),
               "--add", str(a.add)] + (["--lib", a.parent_lib] if tag == "parent" else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
        if r.returncode != 0:      # nothing more is started on the device after a failure
            raise SystemExit(f"{kind} {tag}: child failed ({r.returncode})")
        return json.loads(r.stdout.strip().splitlines()[-1])

    def write():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    for tag in ("parent", "new"):
        out["hashes"][tag] = leg(tag, "bytes")
        write()
    differ = sorted(k for k in out["hashes"]["new"] if out["hashes"]["new"][k] != out["hashes"]["parent"].get(k))
    out["hashes_equal"] = not differ and out["hashes"]["new"].keys() == out["hashes"]["parent"].keys()
    out["hashes_that_differ"] = differ
    print(json.dumps({"hashes_equal": out["hashes_equal"], "differ": differ}), flush=True)
    for tag in ("parent", "new", "parent", "new", "parent"):
        rec = leg(tag, "time")
        rec["leg"] = tag
        out["time_legs"].append(rec)
        print(json.dumps(rec), flush=True)
        write()
    out["gate"] = {key: gate(out["time_legs"], key) for key in ("build_seconds", "append_finalize_wall_seconds")}
    print(json.dumps(out["gate"]), flush=True)
    write()
    if not out["hashes_equal"] or not all(g["within_spread"] for g in out["gate"].values()):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
