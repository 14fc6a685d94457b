"""String data (data type 3) on the GPU: leven and bit_hamming k-NN, range search and get_distance against the
reference's fixture (tests/golden/golden_strings.npz) and against the Python restatement (tests/string_ref.py)."""
import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import string_ref
from tests.golden import gen_golden_strings as gs
from tests.test_strings_cpu import SETS, gst, ref_distance  # noqa: F401  (gst: the fixture)

pytestmark = pytest.mark.gpu


def make(space, rows, method="seq_search", ids=None):
    idx = nz.Index(space, method, data_type="ObjectAsString", dist_type="Int")
    idx.addStringBatch(rows, ids=ids)
    idx.buildIndex()
    return idx


def popcount_matrix(R, Q):
    """R [n][W], Q [q][W] uint32 -> [q][n] Hamming distances"""
    x = np.bitwise_xor(Q[:, None, :], R[None, :, :])
    return np.unpackbits(x.view(np.uint8), axis=-1).sum(axis=-1).astype(np.int64)


@pytest.mark.parametrize("method", ["brute_force", "seq_search"])
@pytest.mark.parametrize("tag", sorted(SETS))
def test_knn_matches_reference(gst, tag, method):
    space, rows, qs = SETS[tag]
    idx = make(space, rows, method)
    for k in (10, 100):
        ids, ds, cnt = idx.knnQueryBatch(qs, k)
        m = min(k, len(rows))
        np.testing.assert_array_equal(cnt, np.full(len(qs), m))
        np.testing.assert_array_equal(ids[:, :m], gst[f"{tag}_k{k}_ids"][:, :m], err_msg=f"{tag} k={k}")
        np.testing.assert_array_equal(ds[:, :m], gst[f"{tag}_k{k}_dists"][:, :m])
    i1, d1 = idx.knnQuery(qs[0], 10)                      # the one-query entry: same lists
    np.testing.assert_array_equal(i1, gst[f"{tag}_k10_ids"][0, :len(i1)])
    idx.close()


@pytest.mark.parametrize("tag", sorted(SETS))
def test_range_and_get_distance_match_reference(gst, tag):
    space, rows, qs = SETS[tag]
    idx = make(space, rows)
    for cap in gs.RANGE_CAPS:
        at = 0
        rn = gst[f"{tag}_range{cap}_n"]
        for qi, q in enumerate(qs):
            for j, rad in enumerate(gst[f"{tag}_radii"][qi]):
                rid, rd = idx.rangeQueryFill(q, float(rad), cap)
                c = rn[2 * qi + j]
                np.testing.assert_array_equal(rid, gst[f"{tag}_range{cap}_ids"][at:at + c], err_msg=f"{tag} q{qi}")
                np.testing.assert_array_equal(rd, gst[f"{tag}_range{cap}_dists"][at:at + c])
                at += c
    got = np.array([idx.getDistance(int(a), int(b)) for a, b in gst[f"{tag}_pairs"]], np.float32)
    np.testing.assert_array_equal(got, gst[f"{tag}_pair_dists"])
    idx.close()


def test_query_lengths_across_block_and_stage_limits():
    """Queries of 1, 63, 64, 65, 200 and 600 bytes (one block, two, four, ten: the multi-block state in LDS and in HBM)
    over rows of 1-700 bytes (256-row chunks that do and do not fit the LDS row stage)."""
    rng = np.random.default_rng(3)
    alpha = np.frombuffer(b"acgt", np.uint8)
    rows = [gs._rand_str(rng, 1, 90, alpha) for _ in range(700)] + [gs._rand_str(rng, 300, 700, alpha) for _ in range(300)]
    rng.shuffle(rows)
    qs = [gs._rand_str(rng, m, m, alpha) for m in (1, 63, 64, 65, 200, 600)]
    idx = make("leven", rows)
    for q in qs:
        want_i, want_d = string_ref.knn(lambda i: string_ref.levenshtein(rows[i], q), len(rows), 25)
        ids, ds = idx.knnQuery(q, 25)
        np.testing.assert_array_equal(ids, want_i, err_msg=f"len {len(q)}")
        np.testing.assert_array_equal(ds, want_d.astype(np.float32))
        rad = float(want_d[-1])
        rid, rd = idx.rangeQueryFill(q, rad, 2000)
        d = np.array([string_ref.levenshtein(r, q) for r in rows])
        np.testing.assert_array_equal(rid, np.nonzero(d <= rad)[0])
        np.testing.assert_array_equal(rd, d[d <= rad].astype(np.float32))
    for a, b in ((0, 1), (5, 900), (int(np.argmax([len(r) for r in rows])), 3)):
        assert idx.getDistance(a, b) == string_ref.levenshtein(rows[a], rows[b])
    idx.close()


@pytest.mark.parametrize("bits", [64, 1000])
def test_large_k_and_batch_slicing(bits):
    """k = 4100 over 20 000 rows with 1700 queries: the per-split lists exceed one slice, so the batch is cut."""
    rng = np.random.default_rng(bits)
    n, nq, k = 20000, 1700 if bits == 64 else 40, 4100
    B = rng.integers(0, 2, size=(n, bits))
    QB = rng.integers(0, 2, size=(nq, bits))
    text = lambda v: " ".join(map(str, v.tolist()))         # noqa: E731
    rows = [text(v) for v in B]
    qs = [text(v) for v in QB]
    R = np.array([string_ref.bit_object(r)[:-1] for r in rows])
    Q = np.array([string_ref.bit_object(q)[:-1] for q in qs])
    idx = make("bit_hamming", rows, "brute_force")
    ids, ds, cnt = idx.knnQueryBatch(qs, k)
    assert (cnt == k).all()
    for qi in range(0, nq, max(1, nq // 60)):
        d = popcount_matrix(R, Q[qi:qi + 1])[0]
        o = np.lexsort((np.arange(n), d))[:k]
        np.testing.assert_array_equal(ids[qi], o, err_msg=f"query {qi}")
        np.testing.assert_array_equal(ds[qi], d[o].astype(np.float32))
    idx.close()


def test_large_k_leven_and_k_above_n():
    rng = np.random.default_rng(11)
    alpha = np.frombuffer(b"ab", np.uint8)
    rows = [gs._rand_str(rng, 1, 10, alpha) for _ in range(5000)]
    qs = [gs._rand_str(rng, 5, 5, alpha) for _ in range(3)] + [gs._rand_str(rng, 100, 100, alpha)]
    idx = make("leven", rows)
    for q in qs:
        for k in (4097, 6000):
            want_i, want_d = string_ref.knn(lambda i: string_ref.levenshtein(rows[i], q), len(rows), k)
            ids, ds = idx.knnQuery(q, k)
            np.testing.assert_array_equal(ids, want_i)
            np.testing.assert_array_equal(ds, want_d.astype(np.float32))
    idx.close()


def test_determinism_external_ids_and_memory_usage():
    rng = np.random.default_rng(8)
    rows = [gs._rand_str(rng, 1, 64, gs.PRINTABLE) for _ in range(3000)]
    qs = [gs._rand_str(rng, 20, 20, gs.PRINTABLE) for _ in range(40)]
    ext = (np.arange(len(rows)) * 7 + 100).astype(np.int32)
    idx = nz.Index("leven", "seq_search", data_type="ObjectAsString", dist_type="Int")
    idx.addStringBatch(rows, ids=ext)
    idx.buildIndex(gpu_defer=1)
    host = nz.lib().nmslib_index_memory_usage(idx.h)
    assert host == sum(16 + len(r) for r in rows)
    a = idx.knnQueryBatch(qs, 50)
    b = idx.knnQueryBatch(qs, 50)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    want_i, _ = string_ref.knn(lambda i: string_ref.levenshtein(rows[i], qs[0]), len(rows), 50)
    np.testing.assert_array_equal(a[0][0], ext[want_i])
    hbm = nz.lib().nmslib_index_memory_usage(idx.h) - host
    store = sum(len(r) for r in rows) + (len(rows) + 1) * 8
    assert hbm >= store + 4 * len(rows)                       # the bytes, the offsets and the ids in HBM
    idx.close()


def test_query_errors_return_codes():
    idx = make("bit_hamming", ["0 1 1 0", "1 1 1 1"])
    with pytest.raises(nz.NmslibError) as e:
        idx.knnQuery("0 1 1", 1)                               # bit count differs
    assert e.value.code == 2
    with pytest.raises(nz.NmslibError) as e:
        idx.knnQuery("0 1 5 0", 1)
    assert e.value.code == 9
    with pytest.raises(nz.NmslibError) as e:
        idx.rangeQuery("0 1 1", 3)
    assert e.value.code == 2
    ids, ds = idx.knnQuery("label:4 1,1,1:1", 2)              # a label and separators, as the rows' parser reads them
    assert ids.tolist() == [1, 0] and ds.tolist() == [0.0, 2.0]
    idx.close()
    idx = make("leven", ["hello", "world"])
    with pytest.raises(nz.NmslibError) as e:
        idx.knnQuery("", 1)
    assert e.value.code == 2
    ids, ds = idx.knnQuery("hello", 2)                         # the Zig string workflow's query, over seq_search
    assert ids.tolist() == [0, 1] and ds.tolist() == [0.0, 4.0]
    assert idx.getDataPointString(0) == b"hello\0"
    idx.close()


# ---- HNSW ----------------------------------------------------------------------------------------------------------
def test_zig_string_workflow_through_hnsw(gst):
    """lib.zig:1381-1398: Index.init(..., "leven", null, "hnsw", .ObjectAsString, .Int), addStringBatch, buildIndex,
    knnQuery k = 2, borrowDataPointString(0) -- as the reference answers it."""
    idx = nz.Index("leven", "hnsw", data_type="ObjectAsString", dist_type="Int")
    idx.addStringBatch(["hello", "world"])
    idx.buildIndex()
    ids, ds = idx.knnQuery("hello", 2)
    np.testing.assert_array_equal(ids, gst["zig_ids"])
    np.testing.assert_array_equal(ds, gst["zig_dists"])
    assert np.array_equal(np.frombuffer(idx.getDataPointString(0), np.uint8), gst["zig_point0"])
    idx.close()


def test_hnsw_recall_against_reference(gst):
    rows, qs = gs.hnsw_set()
    assert np.array_equal(gs.sha(rows), gst["hnsw_rows_sha"]) and np.array_equal(gs.sha(qs), gst["hnsw_queries_sha"])
    idx = nz.Index("leven", "hnsw", data_type="ObjectAsString", dist_type="Int")
    idx.addStringBatch(rows)
    idx.buildIndex(M=gs.HNSW_M, efConstruction=gs.HNSW_EFC, indexThreadQty=1)
    ids, ds, cnt = idx.knnQueryBatch(qs, gs.HNSW_K)          # efSearch 200, the reference shim's
    assert (cnt == gs.HNSW_K).all()
    for qi in range(0, len(qs), 10):                         # the distances are the true ones
        assert [string_ref.levenshtein(rows[i], qs[qi]) for i in ids[qi]] == ds[qi].tolist()
    rec = gs.recall_at_k(ds, gst["hnsw_exact_dists"])
    assert rec >= float(gst["hnsw_ref_recall"][0]) - 0.01, rec
    idx.close()


@pytest.mark.parametrize("space", ["leven", "bit_hamming"])
@pytest.mark.parametrize("algo,ef", [("v1merge", 20), ("v1merge", 64), ("old", 20), ("hybrid", 1000)])
def test_hnsw_walks_equal_host_restatement(space, algo, ef):
    """GPU search over the engine's own graph = the restated baseSearchAlgorithmV1Merge / Old on the same graph:
    positions, distances and the number of distance computations, query by query (long leven queries included)."""
    from tests.test_strings_cpu import graph_of
    rng = np.random.default_rng(17)
    n = 1500
    if space == "leven":
        alpha = gs.LOWER[:5]
        rows = [gs._rand_str(rng, 2, 14, alpha) for _ in range(n)]
        qs = [gs._rand_str(rng, 6, 6, alpha) for _ in range(10)] + [gs._rand_str(rng, 70, 70, alpha) for _ in range(3)]
        qbytes = qs
    else:
        rows = [" ".join(map(str, rng.integers(0, 2, 96).tolist())) for _ in range(n)]
        qs = [" ".join(map(str, rng.integers(0, 2, 96).tolist())) for _ in range(12)]
        qbytes = [q.encode() for q in qs]
    idx = nz.Index(space, "hnsw", data_type="ObjectAsString", dist_type="Int")
    idx.addStringBatch(rows)
    idx.buildIndex(M=6, efConstruction=40, indexThreadQty=1)
    idx.setQueryTimeParams(efSearch=ef, algoType=algo)
    k = 10
    ids, ds, cnt = idx.knnQueryBatch(qs, k)
    links, ml, ep, _ = graph_of(idx.h, n)
    rbytes = [r.encode() if isinstance(r, str) else r for r in rows]
    for qi, q in enumerate(qbytes):
        if space == "leven":
            dist = lambda v: string_ref.levenshtein(rbytes[v], q)                       # noqa: E731
        else:
            qo = string_ref.bit_object(q)
            dist = lambda v: string_ref.bit_hamming(string_ref.bit_object(rbytes[v]), qo)  # noqa: E731
        want_p, want_d, _ = string_ref.hnsw_search(links, ml, ep, dist, ef, k, old=(algo != "v1merge"))
        assert cnt[qi] == len(want_p)
        np.testing.assert_array_equal(ids[qi, :cnt[qi]], want_p, err_msg=f"{space} {algo} query {qi}")
        np.testing.assert_array_equal(ds[qi, :cnt[qi]], np.array(want_d, np.float32))
    # the counters of the last batch: one knnQuery per query, then ndc against the restatement
    for qi in (0, len(qs) - 1):
        idx.knnQuery(qs[qi], k)
        ndc, hops, _ = idx.read_counters(1)
        q = qbytes[qi]
        if space == "leven":
            dist = lambda v: string_ref.levenshtein(rbytes[v], q)                       # noqa: E731
        else:
            qo = string_ref.bit_object(q)
            dist = lambda v: string_ref.bit_hamming(string_ref.bit_object(rbytes[v]), qo)  # noqa: E731
        assert ndc[0] == string_ref.hnsw_search(links, ml, ep, dist, ef, k, old=(algo != "v1merge"))[2]
        assert hops[0] > 0
    idx.close()
