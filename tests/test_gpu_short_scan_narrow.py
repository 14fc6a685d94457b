"""-m gpu: the narrow tier of the short scan: a filter on 32 rotated columns, exact re-rank of the original
rows.  Whichever tier filters, ids and distances are the bits of the 64-column tier and of the 128-column path."""
import numpy as np
import pytest

from tests import orc, refio
from tests.gpuutil import close_rel, make_index

pytestmark = pytest.mark.gpu

N, D, K = 65536, 128, 10


@pytest.fixture(scope="module")
def lowrank():
    return refio.s_lowrank(N + 130, D, 42), refio.s_lowrank(1024, D, 43)


@pytest.fixture(scope="module")
def gauss():
    return refio.s_gauss(N, D, 42), refio.s_gauss(600, D, 43)


def _err(capfd):
    return capfd.readouterr().err


def _batch(monkeypatch, space, X, Q, short):
    """ids, distances, stats of one batch on a fresh index; short: None (the gates decide), "0", "32" or "64" """
    if short is None:
        monkeypatch.delenv("NMSLIB_GPU_F32_SHORT", raising=False)
    else:
        monkeypatch.setenv("NMSLIB_GPU_F32_SHORT", short)
    idx = make_index(space, "seq_search", X)
    ids, ds, cnt = idx.knnQueryBatch(Q, K)
    st = idx.stats()
    return idx, ids, ds, st


def _served_narrow(err):
    lines = [l for l in err.splitlines() if l.startswith("[short scan] served 1")]
    return bool(lines) and all(l.endswith(" P 32") for l in lines)


@pytest.mark.parametrize("space,nq", [("l2", 256), ("l2", 600), ("negdotprod", 256), ("negdotprod", 600), ("l2", 1024)])
def test_lowrank_rows_take_the_narrow_tier_and_equal_the_other_paths(lowrank, space, nq, monkeypatch, capfd):
    """256 and 600 queries: one group of 32 queries per wave; 1024: two."""
    X, Q = lowrank[0][:N], lowrank[1][:nq]
    monkeypatch.setenv("NMSLIB_GPU_DEBUG", "4096")
    idx, ids, ds, st = _batch(monkeypatch, space, X, Q, None)
    err = _err(capfd)
    assert _served_narrow(err), err
    assert st["last_path"] == 1 and st["fast_tiles_fallback"] == 0, st
    for _ in range(9):   # ten repeats: identical bytes
        i2, d2, _ = idx.knnQueryBatch(Q, K)
        assert i2.tobytes() == ids.tobytes() and d2.tobytes() == ds.tobytes()
    idx.close()
    for other in ("64", "0"):
        capfd.readouterr()
        idx0, ids0, ds0, st0 = _batch(monkeypatch, space, X, Q, other)
        err0 = _err(capfd)
        idx0.close()
        assert st0["last_path"] == 1, st0
        assert ("[short scan] served 1" in err0 and " P 64" in err0) if other == "64" else "[short scan] served 0" in err0, err0
        assert ids.tobytes() == ids0.tobytes() and ds.tobytes() == ds0.tobytes()
    sel = np.r_[0:16, nq - 16:nq]
    opos, odist, _ = orc.seq_search(space, X, Q[sel], K)
    np.testing.assert_array_equal(ids[sel], opos)
    assert close_rel(ds[sel], odist)


@pytest.mark.parametrize("extra", [37, 130])
def test_rows_beyond_n_in_the_last_stage_never_appear(lowrank, extra, monkeypatch, capfd):
    """65 536 + 37 rows: the last stage holds one full set and one partial; + 130: four full and one partial."""
    X, Q = lowrank[0][:N + extra], lowrank[1][:256]
    monkeypatch.setenv("NMSLIB_GPU_DEBUG", "4096")
    idx, ids, ds, st = _batch(monkeypatch, "negdotprod", X, Q, None)
    err = _err(capfd)
    idx.close()
    assert _served_narrow(err) and st["fast_tiles_fallback"] == 0, err
    assert ids.min() >= 0 and ids.max() < len(X)
    Ql = np.ascontiguousarray(np.repeat(X[-8:], 32, axis=0))   # queries whose nearest rows are the last ones: the rows themselves
    idx, ids, ds, st = _batch(monkeypatch, "l2", X, Ql, None)
    err = _err(capfd)
    idx.close()
    assert _served_narrow(err), err
    assert ids.max() < len(X)
    np.testing.assert_array_equal(ids[::32, 0], np.arange(len(X) - 8, len(X)))
    opos, odist, _ = orc.seq_search("l2", X, Ql[::32], K)
    np.testing.assert_array_equal(ids[::32], opos)


def test_padding_columns_do_not_disturb_the_narrow_rotation(monkeypatch, capfd):
    X, Q = refio.s_lowrank(N, 100, 52), refio.s_lowrank(256, 100, 53)
    monkeypatch.setenv("NMSLIB_GPU_DEBUG", "4096")
    idx, ids, ds, st = _batch(monkeypatch, "l2", X, Q, None)
    err = _err(capfd)
    idx.close()
    assert _served_narrow(err) and st["fast_tiles_fallback"] == 0, err
    idx0, ids0, ds0, _ = _batch(monkeypatch, "l2", X, Q, "0")
    idx0.close()
    np.testing.assert_array_equal(ids, ids0)
    np.testing.assert_array_equal(ds, ds0)


def test_gaussian_rows_get_no_tier_and_forced_narrow_falls_back_then_leaves(gauss, monkeypatch, capfd):
    X, Q = gauss
    monkeypatch.setenv("NMSLIB_GPU_DEBUG", "4096")
    idx0, ids0, ds0, _ = _batch(monkeypatch, "l2", X, Q, "0")
    idx0.close()
    capfd.readouterr()
    idx, ids, ds, st = _batch(monkeypatch, "l2", X, Q, None)   # the gates: neither width
    err = _err(capfd)
    idx.close()
    assert "[short scan] served 1" not in err and "gate 1" not in err and " P 32" in err and " P 64" in err, err
    np.testing.assert_array_equal(ids, ids0)
    np.testing.assert_array_equal(ds, ds0)
    idx, ids, ds, st = _batch(monkeypatch, "l2", X, Q, "32")
    err = _err(capfd)
    assert _served_narrow(err), err
    assert st["fast_tiles_fallback"] == st["fast_tiles"], st    # every tile: no room for 2.1 E_s
    np.testing.assert_array_equal(ids, ids0)
    np.testing.assert_array_equal(ds, ds0)
    ids2, ds2, _ = idx.knnQueryBatch(Q, K)                       # (stats() above waited for the first batch)
    err2 = _err(capfd)
    assert "[short scan] served 1" not in err2 and "[short scan] served 0" in err2, err2
    assert idx.stats()["fast_tiles_fallback"] == 0
    np.testing.assert_array_equal(ids2, ids0)
    np.testing.assert_array_equal(ds2, ds0)
    idx.close()


def test_near_duplicate_rows_stay_exact_on_the_narrow_tier(monkeypatch):
    """test_near_duplicate_rows_stay_exact's generator, forced to 32 columns: rows inside each other's E_s -- whatever the
    narrow tiles cannot prove goes to the adaptive kernel."""
    rng = np.random.default_rng(191)
    C = rng.standard_normal((1000, 128)).astype(np.float32)
    X = (np.repeat(C, 80, axis=0) + 1e-3 * rng.standard_normal((80000, 128))).astype(np.float32)
    cq = rng.integers(0, 1000, 600)
    Q = (C[cq] + 1e-3 * rng.standard_normal((600, 128))).astype(np.float32)
    sel = np.r_[0:12, 588:600]
    idx, ids, ds, st = _batch(monkeypatch, "l2", X, Q, "32")
    idx.close()
    opos, odist, _ = orc.seq_search("l2", X, Q[sel], K + 22)
    assert refio.recall_nmslib(ids[sel], opos, odist, K) >= 0.999
    assert close_rel(ds[sel], odist[:, :K], rtol=1e-5, atol=1e-6)
