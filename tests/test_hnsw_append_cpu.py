"""No GPU needed (gpu_defer=1 builds on the host and uploads at first use): the index parameters gpu_append and
gpu_build_cut are parsed and validated where they are served (hnsw over the dense spaces) and stay unknown parameters
everywhere else; the statistics carry rows_appended / rows_uploaded.  The GPU side is tests/test_gpu_hnsw_append.py."""
import pytest

import nmslib_zig_amd as nz
from tests import refio
from tests.gpuutil import make_index

X = refio.s_gauss(120, 8, 3)
WORDS = ["kitten", "sitting", "mitten", "fitting", "bitten", "knitting", "written", "smitten"]


def test_both_keys_are_accepted_on_a_dense_hnsw_index():
    idx = make_index("l2", "hnsw", X, M=4, efConstruction=20, gpu_defer=1, gpu_append=1, gpu_build_cut=100)
    assert idx.graphBuilder() == 1                      # (deferred: the host built it; nothing was appended)
    idx.close()
    idx = make_index("l2", "hnsw", X, M=4, efConstruction=20, gpu_defer=1, gpu_append=0, gpu_build_cut=0)
    idx.close()


@pytest.mark.parametrize("value", [2, -1])
def test_gpu_append_takes_0_or_1(value):
    with pytest.raises(nz.NmslibError) as ei:
        make_index("l2", "hnsw", X, M=4, efConstruction=20, gpu_defer=1, gpu_append=value)
    assert ei.value.code == 8 and "gpu_append" in str(ei.value), ei.value


def test_gpu_build_cut_is_a_position():
    with pytest.raises(nz.NmslibError) as ei:
        make_index("l2", "hnsw", X, M=4, efConstruction=20, gpu_defer=1, gpu_build_cut=-5)
    assert ei.value.code == 8 and "gpu_build_cut" in str(ei.value), ei.value


@pytest.mark.parametrize("method", ["brute_force", "seq_search"])
@pytest.mark.parametrize("key", ["gpu_append", "gpu_build_cut"])
def test_the_exact_scan_refuses_them_as_unknown_parameters(method, key):
    with pytest.raises(nz.NmslibError) as ei:
        make_index("l2", method, X, gpu_defer=1, **{key: 1})
    assert ei.value.code == 8 and "Unknown parameters" in str(ei.value), ei.value


@pytest.mark.parametrize("key", ["gpu_append", "gpu_build_cut"])
def test_a_string_hnsw_index_refuses_them_as_unknown_parameters(key):
    s = nz.Index("leven", "hnsw", data_type="ObjectAsString", dist_type="Int")
    s.addStringBatch(WORDS)
    with pytest.raises(nz.NmslibError) as ei:
        s.buildIndex(M=4, efConstruction=10, indexThreadQty=1, gpu_defer=1, **{key: 1})
    assert ei.value.code == 8 and "Unknown parameters" in str(ei.value), ei.value
    s.close()


def test_stats_carry_the_two_counts():
    idx = make_index("l2", "hnsw", X, M=4, efConstruction=20, gpu_defer=1, gpu_append=1)
    st = idx.stats()
    assert st["rows_appended"] == 0 and st["rows_uploaded"] == 0, st      # nothing has been uploaded yet
    assert list(st)[-2:] == ["rows_appended", "rows_uploaded"]            # appended at the end of the struct
    idx.close()
