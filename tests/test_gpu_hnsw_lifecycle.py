"""-m gpu: a GPU-built HNSW index through sequences of append, delete and consolidate (gpu_build=1, gpu_append=1; DESIGN.md
4.6a - 4.6c), held after EVERY step to a host model of the same sequence (tests/lifecycle_ref.py), list for list.

The model composes the builder's sequential restatement, resumed at the row where an append enters the batch loop
(orc_hnsw_insert_batched), with the numpy restatement of the consolidate's rule, by the engine's own rules for what carries
over: the level stream (an append takes its draws [rows now, rows now + added), the live rows after a consolidate), the
compacted upper-level offsets, the entry point and top level a consolidate leaves.  One driver applies a script to the
index and to the model and compares after every step

  * dataQty, deletedRows, what deleteIds / consolidate return (the lists repaired included), graphBuilder, rows_appended,
  * one batch of 64 queries at efSearch 20 and 64: ids, the distances' bits, counts and the ndc / hops counters of the
    oracle's search on the model's graph, cut to the first k live results (the rule of DESIGN.md 4.6b),
  * wherever no row is marked: the saved file against the model's graph -- levels, offsets, top level, entry point and
    every list with its padding -- its ids and rows, and the index loaded from it against the resident one, bit for bit.

The rows are tests/batched_ref.py's kinds, on which every f32 sum is exact in any order: no tolerance anywhere.  An index
without rows is not searched (after every row was deleted and consolidated away); what is asserted there is the counts and
that the next rows are built in full (rows_appended = 0).

Scripts (lifecycle_ref.scripts; M = 6, efConstruction = 64, gpu_build_batch = 16), each at 300 rows, the smallest of 300 /
600 / 1000 at which the model shows what the script is there for (tests/test_hnsw_lifecycle_ref_cpu.py holds that without a
GPU).  Counters reached (model):

  chain                     build 150, appends of 21, 128 and 1 rows, the second and third starting inside a batch of the
                            append before; batches of up to 16 appended nodes
  append-onto-consolidated  45 of 150 rows deleted and consolidated away, 150 appended onto 105: 24 appended nodes with level
                            >= 1 (the upper offsets grow from the compacted ones), first appended batch 6 nodes
  repair-of-appended        delete, append, consolidate: 229 lists repaired, 128 of them lists of appended nodes
  long                      build, delete, consolidate, append, delete, consolidate, append: 112 and 134 lists repaired, 51 of
                            appended nodes; the second delete marks 25 built and 20 appended rows, one of them under an id
                            that was deleted, consolidated away and added again
  entry-point               the entry point and the whole top level (2) deleted: top level 1 after the consolidate, an
                            appended node raises it to 2 and is the entry point; 23 appended nodes with level >= 1
  small candidate cut       repair-of-appended and long with efConstruction = 8: the consolidate's pools hold up to 35 / 25 and
                            24 candidates and are cut to P = 12
  long on cosinesimil / l2sqr_sift (unit rows / bytes: nearly every comparison is a tie)
  fp16                      append-onto-consolidated with gpu_rows=f16, the appended rows at 8 times the scale
  seeds 1, 3, 5, 6, 10, 11  build of 150 - 250 rows and 8 operations each; together: deletes that mark nothing, consolidates
                            with nothing marked, deletes of everything an append brought, every row deleted, consolidated
                            away and the build in full that follows
"""
import os
import struct
import time

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import batched_ref as br
from tests import lifecycle_ref as lr
from tests import refio
from tests.gpuutil import make_index, same_bits

pytestmark = pytest.mark.gpu

K, NQ, EFS = 10, 64, (20, 64)
N = 300
KIND = {"l2": "d16", "cosinesimil": "unit", "l2sqr_sift": "bytes"}


def index_params(space, params, **more):
    return dict(params, gpu_build=1, gpu_append=1, **({"skip_optimized_index": 1} if space == "l2sqr_sift" else {}), **more)


def queries(space):
    return br.make_rows(KIND[space], NQ, seed=77)


def run(idx, Q, ef, env=None, **qparams):
    """-> (ids, dists, counts), (ndc, hops) of one batch"""
    old = {name: os.environ.get(name) for name in (env or {})}
    os.environ.update(env or {})
    try:
        idx.setQueryTimeParams(efSearch=ef, **qparams)
        res = idx.knnQueryBatch(Q, K)
        ctr = tuple(x.astype(np.int64) for x in idx.read_counters(len(Q))[:2])
    finally:
        for name, v in old.items():
            if v is None:
                del os.environ[name]
            else:
                os.environ[name] = v
    return res, ctr


def assert_expected_search(idx, model, Q, what, env=None, **qparams):
    for ef in EFS:
        want, ndc, hops = model.expected_search(Q, K, ef)
        got, (gndc, ghops) = run(idx, Q, ef, env, **qparams)
        try:
            same_bits(got, want)
            np.testing.assert_array_equal(gndc, ndc, err_msg="ndc")
            np.testing.assert_array_equal(ghops, hops, err_msg="hops")
        except AssertionError as e:
            raise AssertionError(f"{what}, efSearch={ef} {env or ''} {qparams or ''}: {e}") from None


def dat_rows(path, row_bytes):
    """ids and the first row_bytes bytes of every object of a .dat file (space.cc:88-105)"""
    raw = open(path + ".dat", "rb").read()
    (n,) = struct.unpack_from("<Q", raw, 0)
    osz = (len(raw) - 8) // max(n, 1)
    rec = np.frombuffer(raw, np.uint8, n * osz, 8).reshape(n, osz)
    return rec[:, 8:12].copy().view(np.int32).ravel(), rec[:, 24:24 + row_bytes]


def load(path, space):
    if space == "l2sqr_sift":
        return nz.Index.load(path, data_type="DenseUInt8Vector", dist_type="Int")
    return nz.Index.load(path)


class Driver:
    """one script on the index and on the model, compared after every step"""

    def __init__(self, space, X, tmp_path, params=lr.PARAMS, **more):
        self.space, self.X, self.tmp, self.more = space, X, tmp_path, more
        self.params = index_params(space, params, **more)
        self.model = lr.HnswModel(space, **params)
        self.Q, self.idx, self.step, self.saved = queries(space), None, 0, 0
        self.f16 = more.get("gpu_rows") == "f16"

    def add(self, X, ids):
        if X.dtype == np.uint8:
            self.idx.addUInt8Batch(X, ids)
        else:
            self.idx.addDenseBatch(X, ids)
        self.idx.finalize()

    def apply(self, rec):
        """the step the model has just made, on the index"""
        self.step += 1
        what = f"step {self.step} ({rec['op']})"
        idx, m = self.idx, self.model
        if rec["op"] == "build":
            self.idx = idx = make_index(self.space, "hnsw", rec["X"], rec["ids"], **self.params)
            assert idx.stats()["rows_appended"] == 0
        elif rec["op"] == "append":
            self.add(rec["X"], rec["ids"])
            st = idx.stats()
            # (the append ran, not a silent build in full -- but for the build the rule asks for when no graph is left)
            assert st["rows_appended"] == rec["ret"], (what, st)
            assert st["rows_uploaded"] == (rec["rows"] if rec["ret"] else m.n), (what, st)
        elif rec["op"] == "delete":
            assert idx.deleteIds(rec["ids"]) == rec["ret"], what
        else:
            assert idx.consolidate() == rec["ret"], what
        assert idx.dataQty() == m.n and idx.deletedRows() == (0 if m.n == 0 else int(m.dead.sum())), what
        if m.n == 0:
            return
        assert idx.graphBuilder() == 2, what
        assert_expected_search(idx, m, self.Q, what)
        if self.f16:
            assert idx.stats()["last_path"] == 5, what
        if not m.dead.any():
            self.check_file(what)

    def check_file(self, what):
        idx, m = self.idx, self.model
        path = str(self.tmp / f"step{self.step}.idx")
        idx.save(path, save_data=True)
        self.saved += 1
        got, want = refio.parse_index(path), m.graph()
        assert ("links0_raw" in got) == (self.space != "l2sqr_sift")     # (the optimized file carries the padding)
        if self.space == "l2sqr_sift":
            got["ids"], got["payload"] = dat_rows(path, 128)
        try:
            refio.assert_graph_equals_restatement(got, want)
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from None
        ids, rows = dat_rows(path, want["payload"].shape[1])
        np.testing.assert_array_equal(ids, m.ids, err_msg=what)
        np.testing.assert_array_equal(rows, want["payload"], err_msg=what)
        for p in (0, m.n // 2, m.n - 1):
            np.testing.assert_array_equal(idx.getDataPoint(p), m.X[p], err_msg=what)
        loaded = load(path, self.space)
        try:
            assert loaded.dataQty() == m.n
            qparams = dict(gpu_rows="f16") if self.f16 else {}
            for ef in EFS:
                a, b = run(idx, self.Q, ef), run(loaded, self.Q, ef, **qparams)
                same_bits(b[0], a[0])
                for x, y in zip(a[1], b[1]):
                    np.testing.assert_array_equal(x, y, err_msg=what)
            if self.f16:
                assert loaded.stats()["last_path"] == 5
                assert idx.stats()["hbm_bytes"] == loaded.stats()["hbm_bytes"], what
        finally:
            loaded.close()

    def play(self, steps):
        t = time.perf_counter()
        try:
            records = lr.run_script(self.model, self.X, steps, on_step=self.apply)
        except BaseException:
            self.close()
            raise
        print(f"{self.space} {self.more or ''}: {len(steps)} steps, {self.saved} files compared, "
              f"{time.perf_counter() - t:.2f} s")
        return records

    def close(self):
        if self.idx is not None:
            self.idx.close()
            self.idx = None


@pytest.mark.parametrize("name", list(lr.scripts(N)))
def test_script(name, tmp_path):
    d = Driver("l2", br.make_rows("d16", N), tmp_path)
    records = d.play(lr.scripts(N)[name])
    print(name, lr.witness(name, records))
    if name == "long":                                           # both search kernels on the final state
        for mw in ("0", "2"):
            assert_expected_search(d.idx, d.model, d.Q, "final state", env={"NMSLIB_HNSW_MW": mw})
    d.close()


@pytest.mark.parametrize("name", ["repair-of-appended", "long"])
def test_script_with_a_small_candidate_cut(name, tmp_path):
    """efConstruction = 8: the consolidate cuts its pools to P = max(8, maxM0) = 12 candidates, and pools are larger"""
    d = Driver("l2", br.make_rows("d16", N), tmp_path, params=lr.SMALL_CUT)
    records = d.play(lr.scripts(N)[name])
    pools = [r["largest_pool"] for r in records if r["op"] == "consolidate"]
    print(name, lr.witness(name, records), "largest pools", pools)
    assert min(pools) > 12
    d.close()


@pytest.mark.parametrize("space", ["cosinesimil", "l2sqr_sift"])
def test_long_script_on_the_other_spaces(space, tmp_path):
    """cosinesimil: the file of a consolidated graph is written from the device's normalised rows, after an append a mixture
    of compacted rows and rows normalised since; on rows of unit norm the payload is the rows themselves"""
    d = Driver(space, br.make_rows(KIND[space], N), tmp_path)
    print(space, lr.witness("long", d.play(lr.long_script(N))))
    d.close()


def test_fp16_copy_is_compacted_then_grown_and_rescaled(tmp_path):
    """gpu_rows=f16: the consolidate compacts the copy, the append grows it, and the appended rows (8 times the scale) move
    its exponent, so every row is packed again.  The f16 walk must give the f32 walk's bits (the model's, and the index's own
    with gpu_rows=f32), the index loaded from the file the same with its copy packed from scratch, in as many bytes."""
    X = lr.f16_rows(N)
    d = Driver("l2", X, tmp_path, gpu_rows="f16")
    records = d.play(lr.scripts(N)["append-onto-consolidated"])
    print("fp16", lr.witness("append-onto-consolidated", records))
    for ef in EFS:
        for mw in ("2", "0"):
            f16 = run(d.idx, d.Q, ef, env={"NMSLIB_HNSW_MW": mw}, gpu_rows="f16")
            assert d.idx.stats()["last_path"] == 5
            f32 = run(d.idx, d.Q, ef, env={"NMSLIB_HNSW_MW": mw}, gpu_rows="f32")
            assert d.idx.stats()["last_path"] == 4
            same_bits(f16[0], f32[0])
            for x, y in zip(f16[1], f32[1]):
                np.testing.assert_array_equal(x, y)
    d.close()


@pytest.mark.parametrize("seed", lr.SEEDS)
def test_seeded_script(seed, tmp_path):
    d = Driver("l2", br.make_rows("d16", lr.POOL), tmp_path)
    c = lr.random_coverage(d.play(lr.random_script(seed)))
    print(seed, c)
    assert c["appends_onto_a_mutated_graph"] >= 1 and c["consolidates"] >= 1 and d.saved >= 1, c
    d.close()
