"""A host model of a mutable GPU-built HNSW index (gpu_build=1, gpu_append=1): rows are appended,
deleted by id and consolidated, and after every step the model holds the graph the device must hold, list for list.  It
composes the two restatements the suite already trusts -- the batched builder's (tests/batched_ref.py: restate, resume) and
the consolidate's (tests/consolidate_ref.py) -- by the engine's own rules for what carries over from one step to the next.
Test infrastructure only; nothing here needs a GPU.

Also here: the scripts the GPU tests replay (tests/test_gpu_hnsw_lifecycle.py, tests/test_gpu_scan_lifecycle.py) and their
witnesses, which tests/test_hnsw_lifecycle_ref_cpu.py holds without a GPU."""
import numpy as np

from . import batched_ref as br
from . import consolidate_ref, orc

PARAMS = dict(M=6, efConstruction=64, gpu_build_batch=16)
SMALL_CUT = dict(PARAMS, efConstruction=8)       # the consolidate's pools are cut to P = max(8, maxM0) = 12 candidates


def ext_ids(lo, hi):
    """external ids that are no positions"""
    return (5 * np.arange(lo, hi) + 7).astype(np.int32)


def f16_rows(n, seed=12):
    """coordinates k/32 in [-1, 1), D = 16, the second half of the rows times 8: differences are multiples of 2^-5 below 9,
    their squares multiples of 2^-10 below 81, a sum of 16 needs 4 + 7 + 10 = 21 bits <= 24 -- exact in f32 in any order,
    and every coordinate is exact in fp16 at either scale of the copy"""
    X = (np.random.default_rng(seed).integers(-32, 32, (n, 16)) / 32.0).astype(np.float32)
    X[n // 2:] *= np.float32(8)
    return X


class HnswModel:
    """rows, external ids, tombstones and the graph over the first `built` rows (all of them after every operation)"""

    def __init__(self, space, **params):
        self.space, self.params = space, {k: v for k, v in params.items() if k != "skip_optimized_index"}
        assert self.params.get("post", 0) == 0
        self.X = self.ids = self.dead = self.g = None
        self.built = 0
        self.last = None                 # the orc.HnswGraph of the last build / append: its .stats and .batch

    @property
    def n(self):
        return 0 if self.X is None else len(self.X)

    def build(self, X0, ids0):
        self.X, self.ids = np.ascontiguousarray(X0), np.asarray(ids0, np.int32).copy()
        self.dead = np.zeros(len(X0), bool)
        self.last = br.restate(self.space, self.X, **self.params)
        self.g, self.built = self.last.arrays(), len(X0)
        return 0

    def append(self, X1, ids1):
        """-> the rows that go into the graph in place (rows_appended): 0 where the engine builds in full, which it does
        when no graph is left (every row was deleted and consolidated away)"""
        if self.built == 0:
            return self.build(X1, ids1)
        n0, n1 = self.built, self.built + len(X1)
        assert n0 == self.n
        # one level stream for the index: the new rows take its draws [n0, n1), n0 being the rows the graph has now --
        # the live rows after a consolidate, all rows with the tombstoned ones otherwise (Engine::append_rows_gpu)
        levels = orc.random_levels(n1, self.params.get("M", 16))[n0:n1]
        self.X = np.concatenate([self.X, np.ascontiguousarray(X1)])
        self.ids = np.concatenate([self.ids, np.asarray(ids1, np.int32)])
        self.dead = np.concatenate([self.dead, np.zeros(len(X1), bool)])
        self.last = br.resume(self.space, self.X, self.g, n0, levels, **self.params)    # (tombstones are ordinary nodes)
        self.g, self.built = self.last.arrays(), n1
        return len(X1)

    def delete(self, ids):
        """marks every position that carries one of the ids now -> the newly marked"""
        if self.n == 0:
            return 0
        hit = np.isin(self.ids, np.asarray(ids, np.int32)) & ~self.dead
        self.dead |= hit
        return int(hit.sum())

    def consolidate(self):
        """-> (removed, repaired)"""
        removed = 0 if self.n == 0 else int(self.dead.sum())
        if removed == 0:
            return 0, 0
        if removed == self.n:            # nothing is left: rows and graph go, the next rows are built in full
            self.X = self.ids = self.dead = self.g = self.last = None
            self.built = 0
            return removed, 0
        g, repaired = consolidate_ref.restate(self.g, self.X, np.nonzero(self.dead)[0], self.params.get("efConstruction", 200),
                                              self.params.get("delaunay_type", 2), self.space)
        live = ~self.dead
        self.X, self.ids, self.dead = self.X[live], self.ids[live], np.zeros(int(live.sum()), bool)
        self.g, self.built, self.last = g, len(self.X), None
        return removed, repaired

    def graph(self):
        """the graph in the shape of refio.parse_index, with ids and the rows as the file's payload has them"""
        return dict(self.g, ids=self.ids.copy(), payload=self.payload())

    def payload(self):
        """the rows as the optimized index file stores them: cosinesimil normalised (exactly, on rows of unit norm)"""
        return np.ascontiguousarray(self.X).view(np.uint8).reshape(self.n, -1)

    def oracle_graph(self):
        g = self.g
        return orc.HnswGraph.from_arrays(self.space, self.X, g["maxM"], g["maxM0"], g["maxlevel"], g["enterpoint"], g["levels"],
                                         g["links0"], g["up_off"], g["up_links"])

    def expected_search(self, Q, k, ef):
        """With tombstones: the first k live results of the search for k' = max(ef, k), under their ids.
        Without: the search for k itself, as the engine runs it then.  The walk is the same; the two differ where equal
        distances straddle rank k, because the k (or k') closest entries of the walk's array are emitted in the order of
        (distance, position) and a cut to k behind that re-ordering is not the re-ordering of a cut to k.
        -> (ids, distances, counts), ndc, hops of the walk"""
        nq = len(Q)
        ids = np.full((nq, k), -1, np.int32)
        ds = np.full((nq, k), np.inf, np.float32)
        cnt = np.zeros(nq, np.int32)
        if self.built == 0:
            return (ids, ds, cnt), np.zeros(nq, np.int64), np.zeros(nq, np.int64)
        pos, dist, pcnt, ndc, hops = self.oracle_graph().search(Q, max(ef, k) if self.dead.any() else k, ef, optimized=True)
        for q in range(nq):
            p = pos[q, :pcnt[q]]
            keep = np.nonzero(~self.dead[p])[0][:k]
            ids[q, :len(keep)], ds[q, :len(keep)], cnt[q] = self.ids[p[keep]], dist[q, keep], len(keep)
        return (ids, ds, cnt), ndc, hops

    def live_rows(self):
        """rows and ids of the live rows in position order: what an exact scan serves"""
        if self.n == 0:
            return None, np.zeros(0, np.int32)
        return self.X[~self.dead], self.ids[~self.dead]


class ScanModel(HnswModel):
    """the same bookkeeping without a graph (brute_force / seq_search: a consolidate only drops the marked rows)"""

    def build(self, X0, ids0):
        self.X, self.ids = np.ascontiguousarray(X0), np.asarray(ids0, np.int32).copy()
        self.dead = np.zeros(len(X0), bool)
        self.built = len(X0)
        return 0

    def append(self, X1, ids1):
        if self.n == 0:
            return self.build(X1, ids1)
        self.X = np.concatenate([self.X, np.ascontiguousarray(X1)])
        self.ids = np.concatenate([self.ids, np.asarray(ids1, np.int32)])
        self.dead = np.concatenate([self.dead, np.zeros(len(X1), bool)])
        self.built = len(self.X)
        return 0

    def consolidate(self):
        removed = 0 if self.n == 0 else int(self.dead.sum())
        if removed == self.n:
            self.X = self.ids = self.dead = None
            self.built = 0
        elif removed:
            live = ~self.dead
            self.X, self.ids, self.dead = self.X[live], self.ids[live], np.zeros(int(live.sum()), bool)
            self.built = len(self.X)
        return removed, 0


# ---- scripts ------------------------------------------------------------------------------------------------------------
# A script is a list of steps over one pool of rows X (row r has the id ext_ids(r) unless a step says otherwise):
#   ("build", lo, hi)  ("append", lo, hi[, ids])  ("delete", f)  ("consolidate",)
# f(model) -> the ids to delete, computed from the model's state when the step runs.

def positions(sel):
    """delete step: the ids at the positions sel(model) gives"""
    return lambda m: m.ids[np.asarray(sel(m), np.int64)] if m.n else np.zeros(0, np.int32)


def share_of(lo_frac, hi_frac, share, seed):
    """positions: `share` of the positions in [lo_frac * n, hi_frac * n), drawn with `seed`"""
    def sel(m):
        if m.n == 0:
            return np.zeros(0, np.int64)
        lo, hi = int(lo_frac * m.n), int(hi_frac * m.n)
        live = lo + np.nonzero(~m.dead[lo:hi])[0]
        return np.sort(np.random.default_rng(seed).permutation(live)[:int(len(live) * share)])
    return sel


def top_level(m):
    """positions: the entry point and every node of the top level"""
    return np.nonzero(m.g["levels"] == m.g["maxlevel"])[0]


def long_script(n):
    """build, delete, consolidate, append, delete (old and appended rows, and an id that was deleted, consolidated away and
    added again with the append), consolidate, append"""
    a, b = n // 2, (3 * n) // 4
    again = ext_ids(3, 4)                                # row 3's id: deleted with the first delete, row a comes under it
    return [("build", 0, a), ("delete", lambda m: np.r_[positions(share_of(0, 1, 0.3, 41))(m), again]), ("consolidate",),
            ("append", a, b, np.r_[again, ext_ids(a + 1, b)]),
            ("delete", lambda m: np.r_[positions(share_of(0, 1, 0.25, 42))(m), again]), ("consolidate",), ("append", b, n)]


def scripts(n):
    """name -> steps; every one has its witness in `witness`"""
    a = n // 2
    return {
        # cuts inside what would be one batch (batches hold 16 nodes from 256 rows on), the last append of one row
        "chain": [("build", 0, a), ("append", a, a + 21), ("append", a + 21, n - 1), ("append", n - 1, n)],
        "append-onto-consolidated": [("build", 0, a), ("delete", positions(share_of(0, 1, 0.3, 43))), ("consolidate",),
                                     ("append", a, n)],
        "repair-of-appended": [("build", 0, a), ("delete", positions(share_of(0, 1, 0.3, 44))), ("append", a, n),
                               ("consolidate",)],
        "long": long_script(n),
        "entry-point": [("build", 0, a), ("delete", positions(top_level)), ("consolidate",), ("append", a, n)],
    }


def lists_with_a_dead_entry(g, dead, nodes):
    """how many lists of the live nodes among `nodes` hold a deleted node: the lists a consolidate repairs"""
    count = 0
    for u in nodes:
        if not dead[u]:
            count += sum(1 for l in range(int(g["levels"][u]) + 1) if dead[consolidate_ref.adj(g, u, l)].any())
    return count


def largest_pool(g, dead):
    """the most distinct live one-hop candidates the repair of any level-0 list has"""
    best = 0
    for u in np.nonzero(~dead)[0]:
        lst = consolidate_ref.adj(g, u, 0)
        if dead[lst].any():
            cand = set()
            for d in lst[dead[lst]]:
                cand |= {int(w) for w in consolidate_ref.adj(g, int(d), 0) if not dead[w]}
            best = max(best, len(cand - set(lst.tolist()) - {int(u)}))
    return best


def run_script(model, X, steps, on_step=None):
    """apply the steps to the model; on_step(record) after each -> the records: op, what the operation returned, and the
    counters `witness` reads, taken from the model's state around the step"""
    out = []
    appended = np.zeros(0, bool)         # per position: the row came with an append, not with the build
    for step in steps:
        op = step[0]
        rec = dict(op=op)
        if op in ("build", "append"):
            lo, hi = step[1], step[2]
            ids = step[3] if len(step) > 3 else ext_ids(lo, hi)
            n0, had = model.built, model.n
            rec.update(rows=hi - lo, ids=ids, X=X[lo:hi], n0=n0)
            rec["top_before"] = None if model.g is None else int(model.g["maxlevel"])
            rec["ret"] = model.build(X[lo:hi], ids) if op == "build" else model.append(X[lo:hi], ids)
            if rec["ret"] > 0:
                rec["levels"] = model.g["levels"][n0:].copy()
                rec["largest_batch"] = model.last.stats["largest_batch"]
                rec["first_batch"] = int((model.last.batch[n0:, 0] == 1).sum())
            appended = np.r_[appended, np.ones(hi - lo, bool)] if had else np.zeros(hi - lo, bool)
            if model.g is not None:
                rec["top_after"], rec["enterpoint"] = int(model.g["maxlevel"]), int(model.g["enterpoint"])
        elif op == "delete":
            rec["ids"] = np.asarray(step[1](model), np.int32)
            was = None if model.dead is None else model.dead.copy()
            rec["ret"] = model.delete(rec["ids"])
            rec["deleted_appended"] = 0 if was is None else int((model.dead & ~was & appended).sum())
            rec["all_dead"] = model.n > 0 and bool(model.dead.all())
            rec["readded_hit"] = 0 if was is None else int((model.dead & ~was & (model.ids == ext_ids(3, 4)[0])).sum())
        else:
            g, dead = model.g, model.dead
            if g is not None and dead.any() and not dead.all():
                rec["repaired_appended"] = lists_with_a_dead_entry(g, dead, np.nonzero(appended)[0])
                rec["largest_pool"] = largest_pool(g, dead)
                rec["entry_point_deleted"] = bool(dead[g["enterpoint"]])
                rec["top_level_deleted"] = bool(dead[g["levels"] == g["maxlevel"]].all())
                rec["top_before"] = int(g["maxlevel"])
            if dead is not None:
                appended = appended[~dead]
            rec["ret"] = model.consolidate()
        out.append(rec)
        if on_step is not None:
            on_step(rec)
    return out


def witness(name, records):
    """what the script `name` is there for, from the model's own counters -> the counters; raises if one is missed"""
    w = {}
    appends = [r for r in records if r["op"] == "append" and r["ret"] > 0]
    cons = [r for r in records if r["op"] == "consolidate" and r["ret"][0] > 0]
    if name == "chain":
        w = dict(appends=len(appends), last_append_rows=appends[-1]["rows"],
                 largest_appended_batch=max(r["largest_batch"] for r in appends))
        assert w["appends"] == 3 and w["last_append_rows"] == 1 and w["largest_appended_batch"] >= 2, w
    if name in ("append-onto-consolidated", "entry-point"):
        assert records[-1]["op"] == "append" and records[-2]["op"] == "consolidate" and records[-2]["ret"][0] > 0
        w = dict(appended_nodes_level_ge1=int((appends[-1]["levels"] >= 1).sum()), first_batch=appends[-1]["first_batch"])
        assert w["appended_nodes_level_ge1"] >= 1 and w["first_batch"] >= 2, w
    if name == "repair-of-appended":
        w = dict(repaired=cons[-1]["ret"][1], repaired_lists_of_appended_nodes=cons[-1]["repaired_appended"])
        assert w["repaired_lists_of_appended_nodes"] > 0, w
    if name == "entry-point":
        c, r = cons[0], appends[-1]
        w.update(top_before=c["top_before"], top_after_consolidate=r["top_before"], top_after_append=r["top_after"])
        assert c["entry_point_deleted"] and c["top_level_deleted"], c
        assert w["top_after_consolidate"] < w["top_before"] and w["top_after_append"] > w["top_after_consolidate"], w
        assert r["enterpoint"] >= r["n0"]            # an appended node is the entry point now
    if name == "long":
        dels = [r for r in records if r["op"] == "delete"]
        w = dict(appends=len(appends), consolidates=len(cons), repaired=[c["ret"][1] for c in cons],
                 deleted_appended_rows=dels[1]["deleted_appended"], deleted_built_rows=dels[1]["ret"] - dels[1]["deleted_appended"],
                 repaired_lists_of_appended_nodes=cons[1]["repaired_appended"])
        assert [r["op"] for r in records] == ["build", "delete", "consolidate", "append", "delete", "consolidate", "append"]
        assert w["appends"] == 2 and w["consolidates"] == 2 and w["deleted_appended_rows"] > 0 and w["deleted_built_rows"] > 0, w
        assert w["repaired_lists_of_appended_nodes"] > 0 and all(x > 0 for x in w["repaired"]), w
        assert dels[1]["readded_hit"] == 1           # the id added again names one live row: the appended one
    return w


# ---- seeded random scripts ----------------------------------------------------------------------------------------------
SEEDS = (1, 3, 5, 6, 10, 11)
POOL = 700                               # rows a random script draws from; it starts from a build of 150 - 250 of them


def random_script(seed, pool=POOL):
    """8 operations after the build: 5 drawn from append / delete / consolidate with random sizes, then a delete of a share
    of the rows, a consolidate and an append, so that every script ends with an append onto a consolidated graph and in a
    state that can be saved.  The drawn deletes are a random share of the live rows, nothing (an id no row carries), every
    row the last append brought, or every row; a drawn consolidate comes whether or not anything is marked."""
    rng = np.random.default_rng(1000 + seed)
    used = int(rng.integers(150, 251))
    steps, last = [("build", 0, used)], (0, used)
    for _ in range(5):
        op = rng.choice(["append", "delete", "consolidate"], p=[0.4, 0.35, 0.25])
        if op == "append" and used < pool:
            hi = min(pool, used + int(rng.choice([1, 2, 7, 20, 45, 90])))
            steps.append(("append", used, hi))
            last, used = (used, hi), hi
        elif op == "delete":
            kind = rng.choice(["share", "nothing", "last-append", "everything"], p=[0.55, 0.15, 0.2, 0.1])
            if kind == "share":
                steps.append(("delete", positions(share_of(0, 1, float(rng.choice([0.05, 0.3, 0.6])), int(rng.integers(1 << 30)))),
                              kind))
            elif kind == "nothing":
                steps.append(("delete", lambda m: np.array([1], np.int32), kind))      # (ids are 5 r + 7: no row has id 1)
            elif kind == "last-append":
                steps.append(("delete", (lambda lo, hi: lambda m: ext_ids(lo, hi))(*last), kind))
            else:
                steps.append(("delete", lambda m: m.ids.copy() if m.n else np.zeros(0, np.int32), kind))
        else:
            steps.append(("consolidate",))
    hi = min(pool, used + int(rng.integers(20, 60)))
    steps += [("delete", positions(share_of(0, 1, 0.3, int(rng.integers(1 << 30)))), "share"), ("consolidate",),
              ("append", used, hi)]
    return steps


def random_coverage(records):
    """what one replayed random script met -> dict of counts"""
    c = dict(appends_onto_a_mutated_graph=0, consolidates=0, empty_deletes=0, idle_consolidates=0, rebuilds_from_nothing=0,
             all_rows_dead=0)
    mutated = False
    for r in records:
        if r["op"] == "append":
            c["appends_onto_a_mutated_graph"] += int(r["ret"] > 0 and mutated)
            c["rebuilds_from_nothing"] += int(r["ret"] == 0)
            mutated = mutated or r["ret"] > 0
        elif r["op"] == "delete":
            c["empty_deletes"] += int(r["ret"] == 0)
            c["all_rows_dead"] += int(r["all_dead"])
            mutated = mutated or r["ret"] > 0
        elif r["op"] == "consolidate":
            c["consolidates"] += int(r["ret"][0] > 0)
            c["idle_consolidates"] += int(r["ret"][0] == 0)
    return c
