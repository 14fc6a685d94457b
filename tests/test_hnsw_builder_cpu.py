"""No GPU needed (gpu_defer=1 builds on the host and uploads at first use): Index.graphBuilder() /
nmslib_gpu_graph_builder report 1 for the host builder and 0 where no builder ran.  The GPU side of the same
function is in tests/test_gpu_hnsw_build_wide.py."""
import ctypes as C

import pytest

import nmslib_zig_amd as nz
from tests import refio


def build(X, **params):
    idx = nz.Index("l2", "hnsw")
    idx.addDenseBatch(X)
    idx.buildIndex(efConstruction=40, gpu_defer=1, **params)
    return idx


@pytest.mark.parametrize("params", [dict(M=64, indexThreadQty=1), dict(M=64, gpu_build=0), dict(M=16, delaunay_type=3),
                                    dict(M=128), dict(M=16, post=2), dict(M=16)],
                         ids=lambda p: "-".join(f"{k}{v}" for k, v in p.items()))
def test_host_builds_report_the_host_builder(params):
    idx = build(refio.s_gauss(300, 16, 5), **params)
    assert idx.graphBuilder() == 1
    idx.close()


def test_no_builder_before_the_build_after_a_load_and_without_a_graph(tmp_path):
    X = refio.s_gauss(200, 16, 6)
    idx = nz.Index("l2", "hnsw")
    idx.addDenseBatch(X)
    assert idx.graphBuilder() == 0                      # nothing built yet
    idx.buildIndex(M=8, efConstruction=40, gpu_defer=1, indexThreadQty=1)
    assert idx.graphBuilder() == 1
    path = str(tmp_path / "g.idx")
    idx.save(path, save_data=False)
    idx.close()
    loaded = nz.Index.load(path, load_data=False)
    assert loaded.graphBuilder() == 0                   # a graph from a file: no builder ran here
    loaded.close()
    bf = nz.Index("l2", "brute_force")
    bf.addDenseBatch(X)
    bf.buildIndex(gpu_defer=1)
    assert bf.graphBuilder() == 0                       # no graph at all
    bf.close()


def test_graph_builder_rejects_null_arguments():
    L = nz.lib()
    b = C.c_int(7)
    assert L.nmslib_gpu_graph_builder(None, C.byref(b)) == 2    # NMSLIB_ERROR_INVALID_ARGUMENT
    idx = build(refio.s_gauss(50, 8, 7), M=4)
    assert L.nmslib_gpu_graph_builder(idx.h, None) == 2
    idx.close()
