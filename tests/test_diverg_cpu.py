"""No GPU: the divergence spaces at the C ABI (what is created, what is refused and why), the expected-distance helper
(tests/diverg_ref.py) against the reference's outputs (tests/golden/golden_diverg.npz), and the fixture's inputs."""
import ctypes as C
import os

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import diverg_ref
from tests.golden import gen_golden_diverg as gd

GOLDEN = gd.GOLDEN
SPACES = diverg_ref.SPACES


@pytest.fixture(scope="module")
def gdv():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("method", ["seq_search", "brute_force"])
@pytest.mark.parametrize("space", SPACES)
def test_divergence_spaces_are_created(space, method):
    idx = nz.Index(space, method)
    assert idx.getSpaceType() == space and idx.getMethod() == method
    idx.addDenseBatch(np.full((3, 5), 0.2, np.float32))
    assert idx.dataQty() == 3
    idx.close()


@pytest.mark.parametrize("space,method,data_type,dist_type,word", [
    ("jsdivfastapprox", "seq_search", "DenseVector", "Float", "table-lookup"),
    ("jsmetrfastapprox", "brute_force", "DenseVector", "Float", "table-lookup"),
    ("kldivfast", "hnsw", "DenseVector", "Float", "graph"),
    ("jsmetrslow", "hnsw", "DenseVector", "Float", "graph"),
    ("itakurasaitofast", "seq_search", "DenseVector", "Int", "float distance"),
    ("kldivgenfast", "seq_search", "SparseVector", "Float", "dense float"),
    ("jsdivslow", "seq_search", "DenseUInt8Vector", "Float", "dense float"),
])
def test_unserved_combinations_are_space_incompatible_with_a_reason(space, method, data_type, dist_type, word):
    with pytest.raises(nz.NmslibError) as e:
        nz.Index(space, method, data_type=data_type, dist_type=dist_type)
    assert e.value.code == 5 and word in str(e.value)


def deferred(space, rows):
    idx = nz.Index(space, "seq_search")
    idx.addDenseBatch(rows)
    idx.buildIndex(gpu_defer=1)     # created, nothing uploaded: no device needed
    return idx


def test_query_length_mismatch_is_invalid_argument():
    idx = deferred("kldivfast", np.full((4, 6), 0.1, np.float32))
    with pytest.raises(nz.NmslibError) as e:
        idx.knnQueryBatch(np.full((2, 5), 0.2, np.float32), 1)
    assert e.value.code == 2 and "length" in str(e.value)
    with pytest.raises(nz.NmslibError) as e:
        idx.rangeQueryFill(np.full(7, 0.2, np.float32), 1.0, 4)
    assert e.value.code == 2
    idx.close()


def test_gpu_shards_rejected_on_a_divergence_index():
    idx = nz.Index("jsdivfast", "seq_search")
    idx.addDenseBatch(np.full((4, 6), 0.1, np.float32))
    with pytest.raises(nz.NmslibError) as e:
        idx.buildIndex(gpu_shards=2)
    assert e.value.code == 8 and "one GPU" in str(e.value)
    idx.close()


def test_device_entry_and_save_are_refused(tmp_path):
    idx = deferred("kldivgenfastrq", np.full((4, 6), 0.1, np.float32))
    d = C.c_void_p(1)
    assert nz.lib().nmslib_gpu_knn_query_batch_device(idx.h, d, 1, 6, 1, d, d, None, None) == 5
    with pytest.raises(nz.NmslibError) as e:
        idx.save(str(tmp_path / "x.bin"))
    assert e.value.code == 10
    idx.close()


@pytest.mark.parametrize("space", SPACES)
def test_stored_object_is_what_the_reference_builds(gdv, space):
    """CreateObjFromVect: the "fast" spaces store the values and then their logarithms (2 * D floats), the slow ones
    the values"""
    rows, _ = gd.inputs_tiny()
    idx = nz.Index(space, "seq_search")
    idx.addDenseBatch(rows)
    want = gdv[f"{space}_tiny_obj0"]
    assert len(want) == (5 if space in ("kldivgenslow", "jsdivslow", "jsmetrslow") else 10)
    assert idx.getDataPoint(0).tobytes() == want.tobytes()
    idx.close()


def test_fixture_inputs_are_pinned(gdv):
    for z in (False, True):
        assert (gd.sha(gd.main_rows(z)) == gdv[f"main_rows_sha_z{int(z)}"]).all()
        assert (gd.sha(gd.main_queries(z)) == gdv[f"main_queries_sha_z{int(z)}"]).all()
    for D in gd.DIMS:
        assert (gd.sha(gd.dims_rows(D), gd.dims_queries(D)) == gdv[f"dims{D}_sha"]).all()
    assert (gd.sha(*gd.inputs_dups()) == gdv["dups_sha"]).all()
    assert (gd.sha(*gd.inputs_tiny()) == gdv["tiny_sha"]).all()
    rows, qs = gd.main_rows(True), gd.main_queries(True)
    assert rows.shape == (2500, 19) and qs.shape == (33, 19)
    assert ((rows == 0).any(1).sum(), (qs == 0).any(1).sum()) == (5, 2)
    dr, _ = gd.inputs_dups()
    assert len(dr) - len(np.unique(dr, axis=0)) == 50


@pytest.mark.parametrize("space", SPACES)
def test_helper_agrees_with_the_reference_within_the_bound(gdv, space):
    """The proof that (D + 8) * 2^-24 * S is wide enough for the reference alone: every stored reference distance lies
    within it of the float64 helper.  Measured worst ratio |reference - helper| / bound over the whole fixture: 0.39
    (the Jensen-Shannon spaces; itakurasaitofast 0.15, the KL spaces below 0.1): no space needs a wider constant."""
    worst = 0.0

    def check(rows, qs, ids, dists):
        nonlocal worst
        for q in range(len(qs)):
            d, b = diverg_ref.scan(space, rows, qs[q])
            pos = ids[q]
            err = np.abs(diverg_ref.comparable(space, dists[q]) - d[pos])
            assert (err <= b[pos]).all(), (space, q, float((err / b[pos]).max()))
            worst = max(worst, float((err / b[pos]).max()))

    z = space not in gd.NO_ZEROS
    check(gd.main_rows(z), gd.main_queries(z), gdv[f"{space}_k100_ids"], gdv[f"{space}_k100_dists"])
    for D in gd.DIMS:
        check(gd.dims_rows(D), gd.dims_queries(D), gdv[f"{space}_dims{D}_ids"], gdv[f"{space}_dims{D}_dists"])
    check(*gd.inputs_dups(), gdv[f"{space}_dups_ids"], gdv[f"{space}_dups_dists"])
    rows = gd.main_rows(z)
    for (a, b), want in zip(gdv["main_pairs"], gdv[f"{space}_pair_dists"]):
        d, bnd = diverg_ref.pair(space, rows[a], rows[b])
        assert abs(diverg_ref.comparable(space, want) - d) <= bnd
    print(space, "worst |reference - helper| / bound:", worst)


def test_large_k_case_has_few_near_ties():
    """the k = 5000 GPU case compares ids outside groups closer than the bound: at most 1 % of the positions of the
    helper's own list lie in such a group"""
    rows, qs = diverg_ref.bigk_inputs()
    for space in ("kldivfast", "jsdivfast"):
        pos, d, b = diverg_ref.seq_search(space, rows, qs, 5000)
        assert diverg_ref.near_tie_mask(d, b).mean() <= 0.01
