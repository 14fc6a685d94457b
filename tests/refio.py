"""Helpers around the compiled reference (oracle/_ref) and its on-disk formats.

Test infrastructure only.  The formats parsed here are the reference's own:
  * optimized HNSW index: src/method/hnsw.cc:774-806 (writer) / :1025-1074 (reader)
  * object vectors (.dat): src/space.cc:88-105
"""
import json
import os
import struct
import subprocess
import tempfile

import numpy as np

from . import orc

HAVE_REF = os.path.exists(orc.REF_DRIVER) and os.path.exists(orc.REF_LIB)


def parse_optimized_index(path):
    """Parse the 68-byte header + level-0 block + per-node upper links."""
    with open(path, "rb") as f:
        raw = f.read()
    (flag, n, mem_per_obj, off_l0, off_data, maxlevel, enterpoint, maxM, maxM0, dist_func,
     search_method) = struct.unpack_from("<IIQQQiIQQiQ", raw, 0)
    assert flag == 1, "not an optimized index"
    hdr = 68
    blk = np.frombuffer(raw, np.uint8, n * mem_per_obj, hdr).reshape(n, mem_per_obj)
    obj_hdr = blk[:, off_data:off_data + 16].copy()
    ids = obj_hdr[:, 0:4].copy().view(np.int32).ravel()
    datalen = obj_hdr[:, 8:16].copy().view(np.uint64).ravel()
    payload = blk[:, off_data + 16:off_l0].copy()
    links0 = blk[:, off_l0:off_l0 + 4 * (maxM0 + 1)].copy().view(np.int32).reshape(n, maxM0 + 1)
    # unused slots are uninitialised memory in the file: zero them for comparisons
    cols = np.arange(maxM0 + 1)[None, :]
    links0 = np.where(cols <= links0[:, :1], links0, 0).astype(np.int32)
    pos = hdr + n * mem_per_obj
    levels = np.zeros(n, np.int32)
    up_off = np.full(n, -1, np.int64)
    chunks, raw_chunks, cur = [], [], 0
    for i in range(n):
        (nbytes,) = struct.unpack_from("<I", raw, pos)
        pos += 4
        if nbytes:
            lv = nbytes // ((maxM + 1) * 4)
            levels[i] = lv
            arr = np.frombuffer(raw, np.int32, nbytes // 4, pos).reshape(lv, maxM + 1).copy()
            raw_chunks.append(arr.ravel())
            c = np.arange(maxM + 1)[None, :]
            arr = np.where(c <= arr[:, :1], arr, 0).astype(np.int32)
            up_off[i] = cur
            chunks.append(arr.ravel())
            cur += arr.size
            pos += nbytes
    # this repo's library appends a 32-byte trailer naming the space (ignored by the reference)
    assert pos == len(raw) or (pos + 32 == len(raw) and raw[pos:pos + 8] == b"GFXKNNv1")
    # (links0_raw / up_links_raw: the lists as the file has them, padding behind the counts included)
    links0_raw = blk[:, off_l0:off_l0 + 4 * (maxM0 + 1)].copy().view(np.int32).reshape(n, maxM0 + 1)
    return dict(n=n, mem_per_obj=mem_per_obj, off_level0=off_l0, off_data=off_data,
                maxlevel=maxlevel, enterpoint=enterpoint, maxM=maxM, maxM0=maxM0,
                dist_func=dist_func, search_method=search_method, ids=ids, datalen=datalen,
                payload=payload, links0=links0, levels=levels, up_off=up_off, links0_raw=links0_raw,
                up_links_raw=(np.concatenate(raw_chunks) if raw_chunks else np.zeros(0, np.int32)),
                up_links=(np.concatenate(chunks) if chunks else np.zeros(0, np.int32)))


def parse_regular_index(path):
    """Parse the regular (non-optimized) index file, src/method/hnsw.cc:808-840: u32 0, u32 n, i32 maxlevel,
    u32 enterpoint, u64 M, u64 maxM, u64 maxM0; per node u32 level, then per level u32 count and the ids.  -> the keys
    of parse_optimized_index that a graph needs (the file has no padding: the slots behind a count are zero here)."""
    with open(path, "rb") as f:
        raw = f.read()
    flag, n, maxlevel, enterpoint, M, maxM, maxM0 = struct.unpack_from("<IIiIQQQ", raw, 0)
    assert flag == 0, "not a regular index"
    pos = 40
    links0 = np.zeros((n, maxM0 + 1), np.int32)
    levels = np.zeros(n, np.int32)
    up_off = np.full(n, -1, np.int64)
    chunks, cur = [], 0
    for i in range(n):
        (lv,) = struct.unpack_from("<I", raw, pos)
        pos += 4
        levels[i] = lv
        if lv:
            up_off[i] = cur
        for l in range(lv + 1):
            (c,) = struct.unpack_from("<I", raw, pos)
            pos += 4
            assert c <= (maxM0 if l == 0 else maxM), (i, l, c)
            ids = np.frombuffer(raw, np.int32, c, pos)
            pos += 4 * c
            if l == 0:
                links0[i, 0] = c
                links0[i, 1:1 + c] = ids
            else:
                blk = np.zeros(maxM + 1, np.int32)
                blk[0] = c
                blk[1:1 + c] = ids
                chunks.append(blk)
                cur += maxM + 1
    assert pos == len(raw) or (pos + 32 == len(raw) and raw[pos:pos + 8] == b"GFXKNNv1")
    return dict(n=n, M=M, maxlevel=maxlevel, enterpoint=enterpoint, maxM=maxM, maxM0=maxM0, links0=links0,
                levels=levels, up_off=up_off,
                up_links=(np.concatenate(chunks) if chunks else np.zeros(0, np.int32)))


def parse_index(path):
    """either file format, by its first word"""
    with open(path, "rb") as f:
        (flag,) = struct.unpack("<I", f.read(4))
    return parse_optimized_index(path) if flag == 1 else parse_regular_index(path)


def _list_of(g, i, l):
    """adjacency block [count, ids..., padding] of node i on level l in a parsed graph"""
    if l == 0:
        return g["links0"][i]
    o = g["up_off"][i] + (l - 1) * (g["maxM"] + 1)
    return g["up_links"][o:o + g["maxM"] + 1]


class _ParsedGraph:
    """a graph in the keys of parse_index behind what assert_graph_equals_restatement reads of an orc.HnswGraph"""

    def __init__(self, g):
        self.g, self.n = g, int(g["n"])
        self.maxlevel, self.enterpoint, self.maxM, self.maxM0 = (int(g[k]) for k in ("maxlevel", "enterpoint", "maxM", "maxM0"))
        self.batch = g.get("batch", np.zeros((self.n, 2), np.int32))

    def levels(self):
        return self.g["levels"]

    def links0(self):
        return self.g["links0"]

    def flat_upper(self):
        return self.g["up_off"], self.g["up_links"]

    def build_distance(self, a, b):
        return float("nan")


def assert_graph_equals_restatement(got, want):
    """`got`: a parsed index file (parse_index); `want`: the orc.HnswGraph of orc.HnswGraph.build_batched, or a graph in
    the keys of parse_index (then without distances and batches in the message; its ids and payload, where it has them,
    must be the file's too).  Levels, top
    level, entry point, maxM0 and every list of every node on every level must be equal, entry by entry in list order,
    and where the file carries padding behind a count it must be zeros.  On a difference the message names the
    differing node that was inserted first, with its level, its batch and index in the batch, and both lists with the
    distances to the node."""
    if isinstance(want, dict):
        for key in ("ids", "payload"):
            if key in want:
                np.testing.assert_array_equal(got[key], want[key], err_msg=key)
        want = _ParsedGraph(want)
    n = want.n
    assert got["n"] == n
    wl = want.levels()
    np.testing.assert_array_equal(got["levels"], wl, err_msg="levels")
    assert (got["maxlevel"], got["enterpoint"], got["maxM0"], got["maxM"]) == \
        (want.maxlevel, want.enterpoint, want.maxM0, want.maxM), "maxlevel / enterpoint / maxM0 / maxM"
    wup_off, wup = want.flat_upper()
    w = dict(links0=want.links0(), up_off=wup_off, up_links=wup, maxM=want.maxM)
    if "links0_raw" in got:
        raw = got["links0_raw"]
        behind = np.arange(raw.shape[1])[None, :] > raw[:, :1]
        assert not (raw * behind).any(), "level-0 padding behind the count is not zero"
        rawu = got["up_links_raw"].reshape(-1, got["maxM"] + 1)
        behind = np.arange(rawu.shape[1])[None, :] > rawu[:, :1]
        assert not (rawu * behind).any(), "upper-level padding behind the count is not zero"
    same0 = (got["links0"] == w["links0"]).all(axis=1)
    same_up = np.array_equal(got["up_off"], wup_off) and np.array_equal(got["up_links"], wup)
    if same0.all() and same_up:
        return
    bad = []
    for i in range(n):
        for l in range(int(wl[i]) + 1):
            if not np.array_equal(_list_of(got, i, l), _list_of(w, i, l)):
                bad.append((i, l))
    assert bad, "upper-level offsets differ although every list is equal"
    order = want.batch[:, 0].astype(np.int64) * (n + 1) + want.batch[:, 1]
    i, l = min(bad, key=lambda t: (order[t[0]], -t[1]))

    def show(L):
        ids = L[1:1 + L[0]].tolist()
        return "[" + ", ".join(f"{j}:{want.build_distance(i, j):.9g}" for j in ids) + "]" + \
            ("" if not L[1 + L[0]:].any() else f" padding {L[1 + L[0]:].tolist()}")
    raise AssertionError(
        f"{len(bad)} lists differ from the restatement; first inserted: node {i} (level {int(wl[i])}) on level {l}, "
        f"batch {int(want.batch[i, 0])}, index {int(want.batch[i, 1])} in the batch\n"
        f"  built:       {show(_list_of(got, i, l))}\n  restatement: {show(_list_of(w, i, l))}")


def run_ref_driver(space, method, base, queries, k, index_params="", query_params="", threads=1,
                   repeat=1, save=None, load=None, ids=None, workdir=None):
    """Run oracle/_ref/ref_driver; returns (ids [Q,k], dists [Q,k], cnt [Q], ndc [Q], info)."""
    u8 = space == "l2sqr_sift"
    dt = np.uint8 if u8 else np.float32
    base = np.ascontiguousarray(base, dt)
    queries = np.ascontiguousarray(queries, dt)
    own = workdir is None
    tmp = tempfile.mkdtemp(prefix="refdrv_") if own else workdir
    try:
        bp, qp, op = (os.path.join(tmp, x) for x in ("base.bin", "q.bin", "out"))
        base.tofile(bp)
        queries.tofile(qp)
        cmd = [orc.REF_DRIVER, "--space", space, "--method", method, "--data", bp, "--n",
               str(base.shape[0]), "--dim", str(base.shape[1]), "--queries", qp, "--nq",
               str(queries.shape[0]), "--k", str(k), "--out", op, "--threads", str(threads),
               "--repeat", str(repeat), "--index-params", index_params, "--query-params",
               query_params]
        if u8:
            cmd.append("--u8")
        if save:
            cmd += ["--save", save]
        if load:
            cmd += ["--load", load]
        if ids is not None:
            ip = os.path.join(tmp, "ids.i32")
            np.ascontiguousarray(ids, np.int32).tofile(ip)
            cmd += ["--ids", ip]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("ref_driver failed: " + r.stderr)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        nq = queries.shape[0]
        out_ids = np.fromfile(op + ".ids.i32", np.int32).reshape(nq, k)
        out_d = np.fromfile(op + ".dists.f32", np.float32).reshape(nq, k)
        cnt = np.fromfile(op + ".cnt.i32", np.int32)
        ndc = np.fromfile(op + ".ndc.i64", np.int64)
        return out_ids, out_d, cnt, ndc, info
    finally:
        if own:
            import shutil
            shutil.rmtree(tmp, ignore_errors=True)


# Synthetic inputs and the recall measure live in the package (bench.py uses them without the test package)
from nmslib_zig_amd.datasets import approx_equal_ulps, recall_nmslib, s_gauss, s_lowrank, s_sift_like  # noqa: E402,F401
