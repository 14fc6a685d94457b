"""The rule of nmslib_gpu_consolidate restated in numpy on a parsed graph, and what goes with it: the
reader of the regular index file, the comparison of two parsed graphs and the reachability report.  Test infrastructure
only; nothing here needs a GPU.

The distance is the one the builder's restatement measures (orc_hnsw_build_distance, oracle/knn_oracle.c): squared l2 in
float64, 1 - dot over rows normalised once for cosinesimil, the byte formula (norms minus twice the dot product, integers)
for l2sqr_sift.  It is exact on rows with small integer entries and on the kinds of tests/batched_ref.py (make_rows), on
which every f32 sum is exact in any order: there the order by (distance, position) and the selection test cannot differ
from the kernel's."""
import struct

import numpy as np


def parse_regular_index(path):
    """SaveRegularIndexBin (the index file of a space without an optimized form, l2sqr_sift here) -> parse_optimized_index's
    keys, without ids and payload"""
    raw = open(path, "rb").read()
    flag, n, maxlevel, enterpoint, M, maxM, maxM0 = struct.unpack_from("<IIiIQQQ", raw, 0)
    assert flag == 0
    pos = 40
    links0 = np.zeros((n, maxM0 + 1), np.int32)
    levels, up_off, chunks, cur = np.zeros(n, np.int32), np.full(n, -1, np.int64), [], 0
    for i in range(n):
        (lv,) = struct.unpack_from("<I", raw, pos)
        pos += 4
        levels[i] = lv
        blk = np.zeros((lv, maxM + 1), np.int32)
        for l in range(lv + 1):
            (cnt,) = struct.unpack_from("<I", raw, pos)
            row = np.frombuffer(raw, np.int32, cnt, pos + 4)
            pos += 4 + 4 * cnt
            dst = links0[i] if l == 0 else blk[l - 1]
            dst[0], dst[1:1 + cnt] = cnt, row
        if lv:
            up_off[i] = cur
            chunks.append(blk.ravel())
            cur += blk.size
    return dict(n=n, maxlevel=maxlevel, enterpoint=enterpoint, maxM=maxM, maxM0=maxM0, links0=links0, levels=levels,
                up_off=up_off, up_links=np.concatenate(chunks) if chunks else np.zeros(0, np.int32))


def adj(g, u, l):
    if l == 0:
        row = g["links0"][u]
    else:
        off = int(g["up_off"][u]) + (l - 1) * (g["maxM"] + 1)
        row = g["up_links"][off:off + g["maxM"] + 1]
    return row[1:1 + row[0]]


def build_distance(space, rows):
    """-> dist(u, ws): the distances of row u to the rows ws as the builder measures them (float64; integers for u8 rows)"""
    if space == "l2sqr_sift":
        R = np.asarray(rows).astype(np.int64)
        norms = (R * R).sum(1)
        return lambda u, ws: norms[ws] + norms[u] - 2 * (R[ws] @ R[u])
    if space == "cosinesimil":
        X = np.asarray(rows, np.float32)
        ss = (X * X).sum(1, dtype=np.float32)
        scale = np.where(ss != 0, np.float32(1) / np.sqrt(np.where(ss != 0, ss, 1), dtype=np.float32), np.float32(1))
        R = (X * scale[:, None].astype(np.float32)).astype(np.float64)       # normalised once, in f32 (hnsw.h:486-497)
        return lambda u, ws: np.maximum(1.0 - np.clip(R[ws] @ R[u], -1.0, 1.0), 0.0)
    if space != "l2":
        raise ValueError(f"no restatement of the consolidate's distance for {space}")
    R = np.asarray(rows).astype(np.float64)
    return lambda u, ws: ((R[ws] - R[u]) ** 2).sum(1)


def restate(g, rows, dead_pos, efc, delaunay, space="l2"):
    """DESIGN.md 4.6c on the parsed graph `g` over `rows` (build_distance must be exact on them) -> (graph, repaired)"""
    n, maxM, maxM0 = g["n"], g["maxM"], g["maxM0"]
    P = min(max(efc, maxM0), 1024)
    dead = np.zeros(n, bool)
    dead[dead_pos] = True
    newpos = np.cumsum(~dead) - 1
    newpos[dead] = -1
    live = np.nonzero(~dead)[0]
    dist = build_distance(space, rows)

    repaired = 0
    links0 = np.zeros((len(live), maxM0 + 1), np.int32)
    up_off, chunks, cur = np.full(len(live), -1, np.int64), [], 0
    for u in live:
        lv = int(g["levels"][u])
        blk = np.zeros((lv, maxM + 1), np.int32)
        for l in range(lv + 1):
            lst = adj(g, u, l)
            gone = dead[lst]
            new = [int(v) for v in lst]
            if gone.any():
                repaired += 1
                keep, target = [int(v) for v in lst[~gone]], len(lst)
                seen, pool = set(keep) | {int(u)}, []
                for d in lst[gone]:
                    for w in adj(g, int(d), l):          # one hop: a deleted neighbour of a deleted neighbour is not followed
                        if dead[w] or int(w) in seen:
                            continue
                        seen.add(int(w))
                        pool.append(int(w))
                pool = np.array(pool, np.int64)
                dd = dist(u, pool) if len(pool) else np.zeros(0, np.float64)
                order = np.lexsort((pool, dd))[:P]       # ascending by (distance, position), the first P
                rejected = []
                for c, dc in zip(pool[order], dd[order]):
                    if len(keep) >= target:
                        break
                    if delaunay != 0 and keep and (dist(c, np.array(keep)) < dc).any():
                        rejected.append(int(c))
                        continue
                    keep.append(int(c))
                if delaunay == 1:
                    keep += rejected[:target - len(keep)]
                new = keep
            dst = links0[newpos[u]] if l == 0 else blk[l - 1]
            dst[0], dst[1:1 + len(new)] = len(new), newpos[new]
        if lv:
            up_off[newpos[u]] = cur
            chunks.append(blk.ravel())
            cur += blk.size
    enter, top = int(g["enterpoint"]), int(g["maxlevel"])
    if dead[enter]:
        top = int(g["levels"][live].max())
        enter = int(live[g["levels"][live] == top][0])
    out = dict(n=len(live), maxM=maxM, maxM0=maxM0, maxlevel=top, enterpoint=int(newpos[enter]), links0=links0,
               levels=g["levels"][live].copy(), up_off=up_off,
               up_links=np.concatenate(chunks) if chunks else np.zeros(0, np.int32))
    for key in ("ids", "payload"):
        if key in g:
            out[key] = g[key][live]
    return out, repaired


def assert_same_graph(got, want):
    for key in ("n", "maxM", "maxM0", "maxlevel", "enterpoint"):
        assert got[key] == want[key], (key, got[key], want[key])
    for key in ("levels", "up_off", "links0", "up_links", "ids", "payload"):
        if key in want:
            np.testing.assert_array_equal(got[key], want[key], err_msg=key)


def reachability(g):
    """reported, not asserted -> (nodes with an empty list on a level that has more than one node, nodes that a walk over
    the level-0 lists from the entry point does not reach)"""
    n = g["n"]
    empty = 0
    for l in range(int(g["maxlevel"]) + 1):
        on = np.nonzero(g["levels"] >= l)[0]
        if len(on) > 1:
            empty += sum(1 for u in on if len(adj(g, u, l)) == 0)
    seen = np.zeros(n, bool)
    seen[g["enterpoint"]] = True
    frontier = [int(g["enterpoint"])]
    while frontier:
        nxt = np.unique(np.concatenate([adj(g, u, 0) for u in frontier]))
        nxt = nxt[~seen[nxt]]
        seen[nxt] = True
        frontier = nxt.tolist()
    return empty, int(n - seen.sum())
