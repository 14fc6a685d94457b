"""-m gpu: exact k-NN, range search and get_distance over the divergence spaces against the reference's outputs
(tests/golden/golden_diverg.npz) and the float64 helper with its error bound (tests/diverg_ref.py)."""
import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import diverg_ref
from tests.golden import gen_golden_diverg as gd

pytestmark = pytest.mark.gpu

SPACES = diverg_ref.SPACES


@pytest.fixture(scope="module")
def gdv():
    with np.load(gd.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def index(space, rows, **params):
    idx = nz.Index(space, "seq_search")
    idx.addDenseBatch(rows)
    idx.buildIndex(**params)
    return idx


def check_knn(space, rows, qs, got_i, got_d, want_i, want_d):
    """ids equal to the reference's (the fixture's generator asserts that no two of the reference's distances a
    comparison reaches are closer than twice the bound, exact copies of one row apart), distances within the bound"""
    for q in range(len(qs)):
        d, b = diverg_ref.scan(space, rows, qs[q])
        pos = want_i[q]
        print(space, "query", q, "worst |gpu - reference| / bound",
              float((np.abs(diverg_ref.comparable(space, got_d[q]) - diverg_ref.comparable(space, want_d[q])) / b[pos]).max()))
        # the distance at each rank against the reference's at that rank
        assert (np.abs(diverg_ref.comparable(space, got_d[q]) - diverg_ref.comparable(space, want_d[q])) <= b[pos]).all()
        np.testing.assert_array_equal(got_i[q], want_i[q], err_msg=f"{space} query {q}")


@pytest.mark.parametrize("space", SPACES)
def test_knn_matches_reference(gdv, space):
    z = space not in gd.NO_ZEROS
    rows, qs = gd.main_rows(z), gd.main_queries(z)
    idx = index(space, rows)
    assert idx.stats()["hbm_bytes"] >= len(rows) * 2 * rows.shape[1] * 4
    for k in (10, 100):
        ids, ds, cnt = idx.knnQueryBatch(qs, k)
        np.testing.assert_array_equal(cnt, gdv[f"{space}_k{k}_cnt"])
        check_knn(space, rows, qs, ids, ds, gdv[f"{space}_k{k}_ids"], gdv[f"{space}_k{k}_dists"])
    idx.close()
    for D in gd.DIMS:
        rows, qs = gd.dims_rows(D), gd.dims_queries(D)
        idx = index(space, rows)
        ids, ds, cnt = idx.knnQueryBatch(qs, 10)
        assert (cnt == 10).all()
        check_knn(space, rows, qs, ids, ds, gdv[f"{space}_dims{D}_ids"], gdv[f"{space}_dims{D}_dists"])
        idx.close()
    rows, qs = gd.inputs_dups()                       # 50 exact copies: (distance, position) order, bit-equal ties
    idx = index(space, rows)
    ids, ds, cnt = idx.knnQueryBatch(qs, len(rows))
    assert (cnt == len(rows)).all()
    check_knn(space, rows, qs, ids, ds, gdv[f"{space}_dups_ids"], gdv[f"{space}_dups_dists"])
    for q in range(len(qs)):
        dup = np.nonzero(ds[q][1:] == ds[q][:-1])[0]   # equal bits: the lower position first
        assert len(dup) >= 50 and (ids[q][dup] < ids[q][dup + 1]).all()
    idx.close()
    rows, qs = gd.inputs_tiny()                       # k = 10 > n = 7
    idx = index(space, rows)
    ids, ds, cnt = idx.knnQueryBatch(qs, 10)
    np.testing.assert_array_equal(ids, gdv[f"{space}_tiny_ids"])
    np.testing.assert_array_equal(cnt, gdv[f"{space}_tiny_cnt"])
    assert (ids[:, 7:] == -1).all() and np.isinf(ds[:, 7:]).all()
    for q in range(len(qs)):
        d, b = diverg_ref.scan(space, rows, qs[q])
        pos = ids[q, :7]
        assert (np.abs(diverg_ref.comparable(space, ds[q, :7]) -
                       diverg_ref.comparable(space, gdv[f"{space}_tiny_dists"][q, :7])) <= b[pos]).all()
    idx.close()


@pytest.mark.parametrize("space", SPACES)
def test_range_and_get_distance_match_reference(gdv, space):
    """The radii are reference distances, so a row lies exactly on each one: the results equal the fixture, or differ
    first at a row whose distance is within the bound of the radius."""
    z = space not in gd.NO_ZEROS
    rows, qs = gd.main_rows(z), gd.main_queries(z)
    pairs = gdv["main_pairs"]
    idx = index(space, rows)
    radii = gdv[f"{space}_radii"]
    for cap in gd.RANGE_CAPS:
        want_n = gdv[f"{space}_range{cap}_n"]
        off = np.concatenate([[0], np.cumsum(want_n)])
        want_i, want_d = gdv[f"{space}_range{cap}_ids"], gdv[f"{space}_range{cap}_dists"]
        c = 0
        for qi in range(len(qs)):
            d, b = diverg_ref.scan(space, rows, qs[qi])
            for r in radii[qi]:
                gi, gdist = idx.rangeQueryFill(qs[qi], r, cap)
                wi, wd = want_i[off[c]:off[c + 1]], want_d[off[c]:off[c + 1]]
                assert (np.diff(gi) > 0).all() and len(gi) <= cap
                if not (len(gi) == len(wi) and (gi == wi).all()):
                    m = min(len(gi), len(wi))
                    j = next((t for t in range(m) if gi[t] != wi[t]), m)
                    at = [lst[j] for lst in (gi, wi) if j < len(lst)]
                    rc = float(diverg_ref.comparable(space, np.float32(r)))
                    assert any(abs(d[p] - rc) <= b[p] for p in at), (space, qi, r)
                m = min(len(gi), len(wi))
                same = gi[:m] == wi[:m]
                # reported: d(query, row)
                for p, g, w in zip(gi[:m][same], gdist[:m][same], wd[:m][same]):
                    _, bb = diverg_ref.pair(space, qs[qi], rows[p])
                    assert abs(diverg_ref.comparable(space, g) - diverg_ref.comparable(space, w)) <= bb
                c += 1
    for (a, b), want in zip(pairs, gdv[f"{space}_pair_dists"]):
        got = idx.getDistance(int(a), int(b))
        dd, bnd = diverg_ref.pair(space, rows[a], rows[b])
        assert abs(diverg_ref.comparable(space, got) - diverg_ref.comparable(space, want)) <= bnd
        if a == b and space != "itakurasaitofast":
            assert abs(diverg_ref.comparable(space, got)) <= bnd          # d(p, p) = 0 for the KL and JS families
    idx.close()


@pytest.mark.parametrize("rq,plain", [("kldivfastrq", "kldivfast"), ("kldivgenfastrq", "kldivgenfast")])
def test_rq_is_the_twin_with_arguments_exchanged(rq, plain):
    rows = gd.main_rows(True)[:40]
    a, b = index(rq, rows), index(plain, rows)
    rng = np.random.default_rng(3)
    for p1, p2 in rng.integers(0, 40, size=(30, 2)).tolist() + [[3, 3], [3, 5]]:
        assert np.float32(a.getDistance(p1, p2)).tobytes() == np.float32(b.getDistance(p2, p1)).tobytes()
    # ... and in a scan: d_rq(row, query) = d_plain(query, row)
    ids, ds, _ = a.knnQueryBatch(rows[7:8], 40)
    for i, d in zip(ids[0], ds[0]):
        assert d.tobytes() == np.float32(b.getDistance(7, int(i))).tobytes()
    a.close()
    b.close()


@pytest.mark.parametrize("space", ["kldivfast", "kldivgenfastrq", "itakurasaitofast", "jsmetrfast", "kldivgenslow"])
def test_batch_independence_bit_for_bit(space):
    """a distance does not depend on the batch, tile or split it was evaluated in"""
    z = space not in gd.NO_ZEROS
    rows, qs = gd.main_rows(z), gd.main_queries(z)
    idx = index(space, rows)
    one = idx.knnQueryBatch(qs, 10)
    again = idx.knnQueryBatch(qs, 10)
    rng = np.random.default_rng(8)
    filler = gd.histograms(rng, 600, rows.shape[1])
    big = idx.knnQueryBatch(np.concatenate([filler, qs]), 10)
    for x, y, w in zip(one[:2], again[:2], big[:2]):
        assert x.tobytes() == y.tobytes()
        assert x.tobytes() == w[600:].tobytes()
    for q in range(len(qs)):
        i, d = idx.knnQuery(qs[q], 10)
        assert i.tobytes() == one[0][q].tobytes() and d.tobytes() == one[1][q].tobytes()
    # ... nor on the entry: the scan, the range filter's array and get_distance agree on d(row, query)
    rows2 = np.concatenate([rows, qs[:1]])
    idx2 = index(space, rows2)
    ids2, ds2, _ = idx2.knnQueryBatch(qs[:1], 50)
    for i, d in zip(ids2[0][:50], ds2[0][:50]):
        assert d.tobytes() == np.float32(idx2.getDistance(int(i), len(rows))).tobytes()
    idx.close()
    idx2.close()


@pytest.mark.parametrize("space", ["kldivfast", "jsdivfast"])
def test_k_above_the_split_list_limit(space):
    """k = 5000 > kScanMaxKl = 4096: a split holds at most 4096 rows and keeps all of them"""
    rows, qs = diverg_ref.bigk_inputs()
    idx = index(space, rows)
    ids, ds, cnt = idx.knnQueryBatch(qs, 5000)
    pos, d, b = diverg_ref.seq_search(space, rows, qs, 5000)
    assert (cnt == 5000).all()
    assert (np.abs(diverg_ref.comparable(space, ds) - d) <= b).all()
    ties = diverg_ref.near_tie_mask(d, b)
    assert ties.mean() <= 0.01
    assert (ids[~ties] == pos[~ties]).all()
    # k = 300: sixteen key buffers of 1024 keys, the largest tile of queries a workgroup keeps in LDS
    ids, ds, cnt = idx.knnQueryBatch(qs, 300)
    assert (cnt == 300).all() and (np.abs(diverg_ref.comparable(space, ds) - d[:, :300]) <= b[:, :300]).all()
    assert (ids[~ties[:, :300]] == pos[:, :300][~ties[:, :300]]).all()
    idx.close()


def test_out_of_domain_inputs_return_k_results():
    """zeros and negative entries give inf / NaN in the reference too: k results, no fault; their order is unspecified"""
    rng = np.random.default_rng(12)
    rows = rng.uniform(-0.2, 1.0, size=(500, 7)).astype(np.float32)
    rows[::9, 2] = 0.0
    for space in ("itakurasaitofast", "kldivgenslow", "kldivfast", "jsdivslow"):
        idx = index(space, rows)
        ids, ds, cnt = idx.knnQueryBatch(rows[:5], 20)
        assert (cnt == 20).all() and (ids >= 0).all() and all(len(set(r)) == 20 for r in ids.tolist())
        idx.close()
