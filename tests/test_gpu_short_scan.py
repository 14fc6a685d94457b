"""-m gpu: the short scan of the exact f32 path: a filter on 64 rotated columns, exact re-rank of the
original rows.  Whichever tier filters, ids and distances are the bits of the 128-column path."""
import numpy as np
import pytest

from tests import orc, refio
from tests.gpuutil import close_rel, make_index

pytestmark = pytest.mark.gpu

N, D, K = 65536, 128, 10


@pytest.fixture(scope="module")
def lowrank():
    return refio.s_lowrank(N + 37, D, 42), refio.s_lowrank(600, D, 43)


@pytest.fixture(scope="module")
def gauss():
    return refio.s_gauss(N, D, 42), refio.s_gauss(600, D, 43)


def _served(capfd):
    err = capfd.readouterr().err
    return "[short scan] served 1" in err, err


def _batch(monkeypatch, space, X, Q, short):
    """ids, distances, stats of one batch on a fresh index; short: None (the gates decide), "0" or "1" """
    if short is None:
        monkeypatch.delenv("NMSLIB_GPU_F32_SHORT", raising=False)
    else:
        monkeypatch.setenv("NMSLIB_GPU_F32_SHORT", short)
    idx = make_index(space, "seq_search", X)
    ids, ds, cnt = idx.knnQueryBatch(Q, K)
    st = idx.stats()
    return idx, ids, ds, st


@pytest.mark.parametrize("nq", [256, 600])
@pytest.mark.parametrize("space", ["l2", "negdotprod"])
def test_lowrank_rows_are_served_and_equal_the_128_column_path(lowrank, space, nq, monkeypatch, capfd):
    X, Q = lowrank[0][:N], lowrank[1][:nq]
    monkeypatch.setenv("NMSLIB_GPU_DEBUG", "4096")
    idx, ids, ds, st = _batch(monkeypatch, space, X, Q, None)
    served, err = _served(capfd)
    assert served, err
    assert st["last_path"] == 1 and st["fast_tiles_fallback"] == 0, st
    # ten repeats: identical bytes
    for _ in range(9):
        i2, d2, _ = idx.knnQueryBatch(Q, K)
        assert i2.tobytes() == ids.tobytes() and d2.tobytes() == ds.tobytes()
    idx.close()
    capfd.readouterr()
    idx0, ids0, ds0, st0 = _batch(monkeypatch, space, X, Q, "0")
    served0, err0 = _served(capfd)
    assert not served0 and st0["last_path"] == 1, err0
    idx0.close()
    np.testing.assert_array_equal(ids, ids0)
    np.testing.assert_array_equal(ds, ds0)
    sel = np.r_[0:16, nq - 16:nq]
    opos, odist, _ = orc.seq_search(space, X, Q[sel], K)
    np.testing.assert_array_equal(ids[sel], opos)
    assert close_rel(ds[sel], odist)


def test_gaussian_rows_stay_on_the_128_column_path(gauss, monkeypatch, capfd):
    X, Q = gauss
    monkeypatch.setenv("NMSLIB_GPU_DEBUG", "4096")
    idx, ids, ds, st = _batch(monkeypatch, "l2", X, Q, None)
    served, err = _served(capfd)
    assert not served and "gate 0" in err, err
    idx.close()
    idx0, ids0, ds0, _ = _batch(monkeypatch, "l2", X, Q, "0")
    idx0.close()
    np.testing.assert_array_equal(ids, ids0)
    np.testing.assert_array_equal(ds, ds0)


def test_gaussian_rows_forced_on_fall_back_then_leave_the_tier(gauss, monkeypatch, capfd):
    X, Q = gauss
    idx0, ids0, ds0, _ = _batch(monkeypatch, "l2", X, Q, "0")
    idx0.close()
    monkeypatch.setenv("NMSLIB_GPU_DEBUG", "4096")
    capfd.readouterr()
    idx, ids, ds, st = _batch(monkeypatch, "l2", X, Q, "1")
    served, err = _served(capfd)
    assert served, err
    assert st["fast_tiles_fallback"] == st["fast_tiles"], st    # every tile: no room for 2.1 E_s
    np.testing.assert_array_equal(ids, ids0)
    np.testing.assert_array_equal(ds, ds0)
    ids2, ds2, _ = idx.knnQueryBatch(Q, K)                       # (stats() above waited for the first batch)
    served2, err2 = _served(capfd)
    assert not served2 and "[short scan] served 0" in err2, err2
    assert idx.stats()["fast_tiles_fallback"] == 0
    np.testing.assert_array_equal(ids2, ids0)
    np.testing.assert_array_equal(ds2, ds0)
    idx.close()


def test_rows_beyond_n_in_the_last_set_never_appear(lowrank, monkeypatch, capfd):
    X, Q = lowrank[0], lowrank[1][:256]
    monkeypatch.setenv("NMSLIB_GPU_DEBUG", "4096")
    idx, ids, ds, st = _batch(monkeypatch, "negdotprod", X, Q, None)
    served, err = _served(capfd)
    assert served and st["fast_tiles_fallback"] == 0, err
    idx.close()
    assert ids.min() >= 0 and ids.max() < len(X)
    # queries whose nearest rows are the last ones: the rows themselves
    Ql = np.ascontiguousarray(np.repeat(X[-8:], 32, axis=0))
    idx, ids, ds, st = _batch(monkeypatch, "l2", X, Ql, None)
    idx.close()
    assert ids.max() < len(X)
    np.testing.assert_array_equal(ids[::32, 0], np.arange(len(X) - 8, len(X)))
    opos, odist, _ = orc.seq_search("l2", X, Ql[::32], K)
    np.testing.assert_array_equal(ids[::32], opos)


def test_padding_columns_do_not_disturb_the_rotation(monkeypatch, capfd):
    X, Q = refio.s_lowrank(N, 100, 52), refio.s_lowrank(256, 100, 53)
    monkeypatch.setenv("NMSLIB_GPU_DEBUG", "4096")
    idx, ids, ds, st = _batch(monkeypatch, "l2", X, Q, None)
    served, err = _served(capfd)
    assert served and st["fast_tiles_fallback"] == 0, err
    idx.close()
    idx0, ids0, ds0, _ = _batch(monkeypatch, "l2", X, Q, "0")
    idx0.close()
    np.testing.assert_array_equal(ids, ids0)
    np.testing.assert_array_equal(ds, ds0)


def test_near_duplicate_rows_stay_exact(monkeypatch):
    """test_f32_fast_path_near_duplicates_stay_exact's generator at 128 columns (the tier needs more than 64), forced on:
    rows inside each other's E_s -- whatever the short tiles cannot prove goes to the adaptive kernel."""
    rng = np.random.default_rng(191)
    C = rng.standard_normal((1000, 128)).astype(np.float32)
    X = (np.repeat(C, 80, axis=0) + 1e-3 * rng.standard_normal((80000, 128))).astype(np.float32)
    cq = rng.integers(0, 1000, 600)
    Q = (C[cq] + 1e-3 * rng.standard_normal((600, 128))).astype(np.float32)
    sel = np.r_[0:12, 588:600]
    idx, ids, ds, st = _batch(monkeypatch, "l2", X, Q, "1")
    idx.close()
    opos, odist, _ = orc.seq_search("l2", X, Q[sel], K + 22)
    assert refio.recall_nmslib(ids[sel], opos, odist, K) >= 0.999
    assert close_rel(ds[sel], odist[:, :K], rtol=1e-5, atol=1e-6)
