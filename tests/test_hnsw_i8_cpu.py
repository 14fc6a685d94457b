"""No GPU: gpu_rows=i8 (the 8-bit traversal copy) as an index and a query-time parameter through the C ABI,
on indexes whose upload is deferred: what is accepted, and every refusal with its code and its reason."""
import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests.gpuutil import make_index

X = np.random.default_rng(5).standard_normal((60, 12)).astype(np.float32)
HNSW = dict(M=6, efConstruction=20, indexThreadQty=1, gpu_defer=1)


def refused(fn, *needles):
    with pytest.raises(nz.NmslibError) as ei:
        fn()
    assert ei.value.code == 2, ei.value                      # NMSLIB_ERROR_INVALID_ARGUMENT
    for s in needles:
        assert s in str(ei.value), ei.value


@pytest.mark.parametrize("space", ["l2", "l1", "cosinesimil", "angulardist", "negdotprod"])
def test_i8_is_accepted_for_the_five_spaces_and_round_trips(space):
    idx = make_index(space, "hnsw", X, gpu_rows="i8", **HNSW)
    for rows in ("f32", "f16", "i8"):
        idx.setQueryTimeParams(efSearch=40, gpu_rows=rows, gpu_rerank=25)
    idx.setQueryTimeParams(efSearch=40)                          # the extensions stay as set
    idx.close()
    idx = make_index(space, "hnsw", X, gpu_rows="f16", **HNSW)
    idx.setQueryTimeParams(gpu_rows="i8")
    idx.close()


def string_index():
    s = nz.Index("leven", "hnsw", data_type="ObjectAsString", dist_type="Int")
    s.addStringBatch(["kitten", "sitting", "mitten", "fitting", "bitten", "knitting", "written", "smitten"])
    return s


REFUSALS = {
    "linf": (lambda: make_index("linf", "hnsw", X, gpu_rows="i8", **HNSW), ("linf", "serves hnsw over l2, l1")),
    "l2sqr_sift": (lambda: make_index("l2sqr_sift", "hnsw", np.zeros((40, 128), np.uint8), gpu_rows="i8", **HNSW),
                   ("l2sqr_sift", "uint8")),
    "string": (lambda: string_index().buildIndex(M=4, efConstruction=10, indexThreadQty=1, gpu_defer=1, gpu_rows="i8"),
               ("string", "float rows")),
    "brute_force": (lambda: make_index("l2", "brute_force", X, gpu_defer=1, gpu_rows="i8"), ("brute_force", "exact scan")),
    "seq_search": (lambda: make_index("l2", "seq_search", X, gpu_defer=1, gpu_rows="i8"), ("seq_search", "exact scan")),
    "shards": (lambda: make_index("l2", "hnsw", X, gpu_rows="i8", gpu_shards=2, **HNSW), ("gpu_shards", "one device")),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_i8_is_refused_by_name_where_it_is_not_served(what):
    # (hnsw over sparse rows or a divergence does not exist: such an index is refused before its parameters are read)
    fn, needles = REFUSALS[what]
    refused(fn, "gpu_rows=i8", *needles)


@pytest.mark.parametrize("space,data", [("linf", X), ("l2sqr_sift", np.zeros((40, 128), np.uint8))])
def test_i8_is_refused_at_query_time_too(space, data):
    idx = make_index(space, "hnsw", data, **HNSW)
    refused(lambda: idx.setQueryTimeParams(gpu_rows="i8"), "gpu_rows=i8", space)
    idx.setQueryTimeParams(efSearch=30)                          # the index still takes good values
    idx.close()
    idx = make_index("l2", "hnsw", X, gpu_shards=2, **HNSW)
    refused(lambda: idx.setQueryTimeParams(gpu_rows="i8"), "gpu_rows=i8", "gpu_shards")
    idx.close()


def test_unknown_values_are_still_refused_and_good_ones_taken_afterwards():
    refused(lambda: make_index("l2", "hnsw", X, gpu_defer=1, gpu_rows="bf16"), "gpu_rows", "f32 or f16", "i8", "bf16")
    idx = make_index("l2", "hnsw", X, **HNSW)
    refused(lambda: idx.setQueryTimeParams(gpu_rows="bf16"), "gpu_rows", "f32 or f16", "i8")
    refused(lambda: idx.setQueryTimeParams(gpu_rows="I8"), "gpu_rows")
    idx.setQueryTimeParams(gpu_rows="i8", gpu_rerank=10)
    idx.close()
