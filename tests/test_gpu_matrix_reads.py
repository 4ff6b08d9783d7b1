"""SharedMatrix reads on the GPU: mte_matrix_cells' rowCount / colCount, getCell and dense
ranges over tests/matrix_edges.py's documents, replayed once by one module-scoped engine.

Every expected value comes from the ORACLE's summary (OracleMatrix.snapshot_json, read back with
tests/test_matrix_spec.py's grid / vector_handles / get_cell and matrix_edges.blob_cells) and from the
builders' closed forms (Doc.want_grid, want_handles, want_cells) -- never from the library's own
snapshot_matrix. tests/test_matrix_reads_cpu.py pins, on the oracle alone, the shapes these tests rely on
(vectors of several 64-row walk steps, an unallocated run, removed rows inside the window)."""
import ctypes
import json
import random

import numpy as np
import pytest

from fluidframework_amd import mte
from tests import matrix_edges as me
from tests.oplog import msg
from tests.test_gpu_matrix_edges import Item, edge_items, interleaved, load
from tests.test_matrix import splice_ins
from tests.test_matrix_spec import CASES, build, get_cell, grid, oracle_summary, vector_handles

pytestmark = pytest.mark.gpu

SHAPE, CELL, RECT = mte.MTE_MQ_SHAPE, mte.MTE_MQ_CELL, mte.MTE_MQ_RECT
OK, OUT_OF_RANGE, DOC_FAILED, BAD_QUERY = mte.MTE_MX_OK, mte.MTE_MX_OUT_OF_RANGE, mte.MTE_MX_DOC_FAILED, mte.MTE_MX_BAD_QUERY
NONE = mte.MTE_CELL_NONE
NO_FULL_GRID = ("levels4200", "big65600")   # 17 M and 197 k cells: read by CELLs and bands instead
E_STATE, E_RANGE = -4, -7

_REF = {}


def ref(it):
    """What the oracle's summary says of one matrix (computed once, shared, never changed): the visible
    handles of both vectors (None = unallocated), the cells root, and, on demand, the grid."""
    if it.name not in _REF:
        tree = it.want()["tree"]
        ents = {e["path"]: e["value"] for e in tree["entries"]}
        _REF[it.name] = {"tree": tree, "rows": vector_handles(ents["rows"]), "cols": vector_handles(ents["cols"]),
                         "root": json.loads(ents["cells"]["contents"])[0]}
    return _REF[it.name]


def ref_grid(it):
    r = ref(it)
    if "grid" not in r:
        r["grid"] = grid(r["tree"])
        assert len(r["grid"]) == len(r["rows"])
    return r["grid"]


def ref_cells(it):
    """{(row handle, col handle): value} of the oracle's blob (the big matrices: a get_cell per cell of a
    50 000-cell band would take seconds)."""
    r = ref(it)
    if "cells" not in r:
        r["cells"] = me.blob_cells(r["tree"])
    return r["cells"]


def ref_cell(it, row, col):
    r = ref(it)
    rh, ch = r["rows"][row], r["cols"][col]
    return None if rh is None or ch is None else get_cell(r["root"], rh, ch)


class Values:
    """value id -> parsed JSON, through value_text (cached per loaded batch)."""

    def __init__(self, e):
        self.e, self.t = e, {}

    def __call__(self, v):
        v = int(v)
        if v == NONE:
            return None
        if v not in self.t:
            self.t[v] = json.loads(self.e.value_text(v))
        return self.t[v]

    def rect(self, vals, r, n_rows, n_cols):
        o = int(r["val_off"])
        ids = vals[o:o + n_rows * n_cols]
        assert len(ids) == n_rows * n_cols
        tab = {int(v): self(v) for v in np.unique(ids)}
        return [[tab[int(v)] for v in ids[i * n_cols:(i + 1) * n_cols]] for i in range(n_rows)]


def full_grids(e, items, pairs):
    """One call: a full-grid RECT per matrix (but the two big ones). {name: grid}."""
    todo = [(it, p) for it, p in zip(items, pairs) if it.name not in NO_FULL_GRID]
    q = [(ri, ci, RECT, 0, 0, len(ref(it)["rows"]), len(ref(it)["cols"])) for it, (ri, ci) in todo]
    out, vals = e.matrix_cells(q)
    val = Values(e)
    got = {}
    for (it, _), r, qq in zip(todo, out, q):
        assert r["status"] == OK and (r["row_count"], r["col_count"]) == (qq[5], qq[6]), (it.name, r)
        got[it.name] = val.rect(vals, r, qq[5], qq[6])
    return got


def check_full_grids(e, items, pairs):
    got = full_grids(e, items, pairs)
    for it in items:
        if it.name in NO_FULL_GRID:
            continue
        assert got[it.name] == ref_grid(it), it.name
        if it.doc is not None and it.doc.want_grid is not None:
            assert got[it.name] == it.doc.want_grid, it.name
    return got


def levels_probe(e, items, pairs):
    """The handle-levels matrix and the 65 600-handle one through a band, a strip and CELLs: the answers
    as plain values, compared with the oracle here and between routes by the callers."""
    names = [it.name for it in items]
    val = Values(e)
    out = {}
    it, (ri, ci) = items[names.index("levels4200")], pairs[names.index("levels4200")]
    r = ref(it)
    n = len(r["rows"])
    res, vals = e.matrix_cells([(ri, ci, RECT, 4090, 0, 12, n), (ri, ci, RECT, 0, 60, n, 11)])
    assert [x["status"] for x in res] == [OK, OK]
    out["band"] = val.rect(vals, res[0], 12, n)
    out["strip"] = val.rect(vals, res[1], n, 11)
    cells = ref_cells(it)
    assert out["band"] == [[cells.get((rh, ch)) for ch in r["cols"]] for rh in r["rows"][4090:4102]]
    assert out["strip"] == [[cells.get((rh, ch)) for ch in r["cols"][60:71]] for rh in r["rows"]]
    assert sum(v is not None for row in out["band"] for v in row) >= 12   # the diagonal crosses the band
    bit, (bri, bci) = items[names.index("big65600")], pairs[names.index("big65600")]
    br = ref(bit)
    pos = {h: p for p, h in enumerate(br["rows"])}
    rows = sorted({pos[rh] + d for rh, _ in bit.big["cells"] for d in (-1, 0, 1) if 0 <= pos[rh] + d < len(br["rows"])})
    # the rows the freed range's neighbours moved to, and the vector's last
    rows = sorted(set(rows) | {65532, 65533, 65534, len(br["rows"]) - 1})
    q = [(bri, bci, CELL, p, c) for p in rows for c in range(len(br["cols"]))]
    res, _ = e.matrix_cells(q)
    out["big"] = {}
    for x, (_, _, _, p, c) in zip(res, q):
        assert x["status"] == OK and (x["row_count"], x["col_count"]) == (len(br["rows"]), len(br["cols"]))
        assert (x["row_handle"] or None, x["col_handle"] or None) == (br["rows"][p], br["cols"][c]), (p, c, x)
        out["big"][(p, c)] = val(x["value"])
        assert out["big"][(p, c)] == ref_cell(bit, p, c) == bit.big["cells"].get((br["rows"][p], br["cols"][c])), (p, c)
    assert sum(v is not None for v in out["big"].values()) == len(bit.big["cells"])
    assert any(br["rows"][p] >= 65536 and v is not None for (p, _), v in out["big"].items())
    return out


@pytest.fixture(scope="module")
def batch():
    """One engine, one replay of the whole edge batch."""
    items = interleaved(edge_items())
    e = mte.Engine(0)
    pairs = load(e, items)
    assert e.replay()["failed_docs"] == 0
    assert e.get_info("mx_tables_built") == 0
    yield {"e": e, "items": items, "pairs": pairs, "names": [it.name for it in items]}
    assert e.get_info("downloaded") == 0   # no read made the whole-pool download
    e.close()


@pytest.fixture(scope="module")
def default_answers(batch):
    e, items, pairs = batch["e"], batch["items"], batch["pairs"]
    return {"grids": check_full_grids(e, items, pairs), "levels": levels_probe(e, items, pairs)}


def test_every_matrix_in_one_call(batch):
    """SHAPE for every matrix of the batch in one call, the empty ones included: counts 0 there, and a
    CELL on them is OUT_OF_RANGE."""
    e, items, pairs = batch["e"], batch["items"], batch["pairs"]
    q = [(ri, ci, SHAPE) for ri, ci in pairs] + [(ri, ci, CELL, 0, 0) for ri, ci in pairs]
    out, vals = e.matrix_cells(q)
    assert len(vals) == 0
    n_empty = 0
    for k, it in enumerate(items):
        s, c = out[k], out[len(items) + k]
        want = (len(ref(it)["rows"]), len(ref(it)["cols"]))
        assert s["status"] == OK and (s["row_count"], s["col_count"]) == want, (it.name, s, want)
        assert (c["row_count"], c["col_count"]) == want
        if not it.log and it.summary is None:
            n_empty += 1
            assert want == (0, 0) and c["status"] == OUT_OF_RANGE and c["value"] == NONE, (it.name, c)
        else:
            assert c["status"] == OK and Values(e)(c["value"]) == ref_cell(it, 0, 0), (it.name, c)
    assert n_empty >= 5
    assert e.get_info("downloaded") == 0


def test_full_grids(batch, default_answers):
    """A full-grid RECT per matrix in one call equals grid(oracle tree) and the closed form. The rows
    vectors are 1 367 / 323 / 269 / 652 / 282 output rows (several 64-row steps), cols 2 to 4 wide."""
    got = default_answers["grids"]
    assert set(got) == set(batch["names"]) - set(NO_FULL_GRID)
    for n in ("frag1400", "frag350", "frag300", "spliced700", "spliced560r", "recycle24", "writers70", "writers40"):
        assert len(got[n]) > 20 and 2 <= len(got[n][0]) <= 4 and any(v is not None for row in got[n] for v in row), n
    assert batch["e"].get_info("downloaded") == 0


def test_handle_levels_cells_and_bands(batch, default_answers):
    """4 200 x 4 200, both vectors many steps long: CELLs on the diagonal, the four cells around handles
    16 / 256 / 4 096 on each axis and the builder's one-axis corners, with their handles; the band and the
    strip of levels_probe."""
    e, items, pairs, names = batch["e"], batch["items"], batch["pairs"], batch["names"]
    it, (ri, ci) = items[names.index("levels4200")], pairs[names.index("levels4200")]
    r = ref(it)
    n = len(r["rows"])
    assert n == len(r["cols"]) == 4200 and r["rows"] == it.doc.want_handles["rows"] and r["cols"] == it.doc.want_handles["cols"]
    at = [(p, p) for p in range(n)]
    for b in me.LEVELS:   # handle h sits at position h - 1
        at += [(hr - 1, hc - 1) for hr in (b - 1, b) for hc in (b - 1, b)]
        at += [(hr - 1, hc - 1) for hr in (b, b + 1) for hc in (b, b + 1)]
    at += [(hr - 1, hc - 1) for hr, hc in it.doc.facts["corner"]]
    at += [(0, n - 1), (n - 1, 0), (n - 1, n - 1), (5, 9)]
    out, _ = e.matrix_cells([(ri, ci, CELL, p, c) for p, c in at])
    val = Values(e)
    hits = 0
    for x, (p, c) in zip(out, at):
        assert x["status"] == OK and (x["row_count"], x["col_count"]) == (n, n)
        assert (x["row_handle"], x["col_handle"]) == (r["rows"][p], r["cols"][c]), (p, c, x)
        want = ref_cell(it, p, c)
        assert val(x["value"]) == want == it.doc.want_cells.get((p + 1, c + 1)), (p, c, x)
        hits += want is not None
    assert hits >= n + len(it.doc.facts["corner"])
    lv = default_answers["levels"]
    assert len(lv["band"]) == 12 and len(lv["band"][0]) == n and len(lv["strip"]) == n and len(lv["strip"][0]) == 11


def test_big_handles_from_a_summary(batch, default_answers):
    """Row handles >= 65 536, loaded cells, a freed range straddling 65 536 (levels_probe's CELLs)."""
    big = default_answers["levels"]["big"]
    it = batch["items"][batch["names"].index("big65600")]
    got = {v for v in big.values() if v is not None}
    assert got == set(it.big["cells"].values()) and "cutlo" not in got and "cuthi" not in got


def test_random_cells_in_one_call(batch):
    """2 000 CELLs over all matrices in one call, a tenth of them out of range by one on either axis."""
    e, items, pairs = batch["e"], batch["items"], batch["pairs"]
    rng = random.Random(11)
    q, want = [], []
    for k in range(2000):
        i = rng.randrange(len(items))
        it, (ri, ci) = items[i], pairs[i]
        R, C = len(ref(it)["rows"]), len(ref(it)["cols"])
        if k % 10 == 0 or not R or not C:
            p, c = (R, rng.randrange(C + 1)) if k % 20 == 0 else (rng.randrange(R + 1), C)
            q.append((ri, ci, CELL, p, c))
            want.append(None)
        else:
            p, c = rng.randrange(R), rng.randrange(C)
            q.append((ri, ci, CELL, p, c))
            want.append((it, p, c))
    out, _ = e.matrix_cells(q)
    val = Values(e)
    n_out = n_hit = 0
    for x, w in zip(out, want):
        if w is None:
            assert x["status"] == OUT_OF_RANGE and x["value"] == NONE, x
            n_out += 1
            continue
        it, p, c = w
        r = ref(it)
        assert x["status"] == OK
        assert (x["row_handle"] or None, x["col_handle"] or None) == (r["rows"][p], r["cols"][c]), (it.name, p, c, x)
        got = val(x["value"])
        assert got == ref_cell(it, p, c), (it.name, p, c, x)
        n_hit += got is not None
    assert n_out >= 200 and n_hit > 100
    assert e.get_info("downloaded") == 0


def raw_call(e, q, cap):
    """mte_matrix_cells with a vals buffer of `cap` ids: (return code, *vals_len, results)."""
    q = np.array([tuple(t) + (0,) * (8 - len(t)) for t in q], dtype=mte.CELL_Q_DTYPE)
    out = np.zeros(len(q), dtype=mte.CELL_R_DTYPE)
    vals = np.zeros(max(cap, 1), dtype=np.uint32)
    n = ctypes.c_size_t()
    rc = mte.lib().mte_matrix_cells(e._h, q.ctypes.data, len(q), out.ctypes.data, vals.ctypes.data, cap, ctypes.byref(n))
    return rc, n.value, out


def test_refusals(batch):
    e, items, pairs, names = batch["e"], batch["items"], batch["pairs"], batch["names"]
    ri, ci = pairs[names.index("recycle24")]
    it = items[names.index("recycle24")]
    R, C = len(ref(it)["rows"]), len(ref(it)["cols"])
    n_docs = 2 * len(items)
    q = [(n_docs, ci, SHAPE), (ri, n_docs + 3, CELL, 0, 0), (ri, ci, 3), (ri, ci, RECT, 0, 0, 65536, 32769),
         (ri, ci, CELL, 1, 0), (ri, ci, RECT, 0, 0, R + 1, C), (ri, ci, RECT, 2, 0, 0, C), (ri, ci, RECT, 1, 0, 2, C)]
    out, vals = e.matrix_cells(q)
    assert [int(x["status"]) for x in out] == [BAD_QUERY] * 4 + [OK, OUT_OF_RANGE, OK, OK]
    # the rectangle not wholly inside is laid out and all NONE; the zero-sided one has no ids
    assert len(vals) == (R + 1) * C + 2 * C and out[5]["val_off"] == 0 and out[6]["val_off"] == out[7]["val_off"] == (R + 1) * C
    assert (vals[:(R + 1) * C] == NONE).all()
    val = Values(e)
    assert val.rect(vals, out[7], 2, C) == ref_grid(it)[1:3] and val(out[4]["value"]) == ref_cell(it, 1, 0)
    # vals_cap one short: MTE_E_RANGE with the size still reported
    rc, need, _ = raw_call(e, q[4:], len(vals) - 1)
    assert (rc, need) == (E_RANGE, len(vals))
    rc, need, out2 = raw_call(e, q[4:], len(vals))
    assert (rc, need) == (0, len(vals)) and [int(x["status"]) for x in out2] == [OK, OUT_OF_RANGE, OK, OK]


def test_before_any_replay():
    e = mte.Engine(0)
    try:
        load(e, [Item("recycle24", log=me.recycling().log)])
        rc, _, _ = raw_call(e, [(0, 1, SHAPE)], 0)
        assert rc == E_STATE
        with pytest.raises(mte.MteError):
            e.matrix_cells([(0, 1, SHAPE)])
    finally:
        e.close()


def test_failed_rows_document():
    """A matrix whose rows vector has more than 127 writers inside the window fails its replay: its queries
    are DOC_FAILED while the other matrix of the call still answers."""
    bad = [msg(f"w{k:03d}", k + 1, k, splice_ins("rows", 0, 1), 0) for k in range(130)]
    good = Item("recycle24", log=me.recycling().log, doc=me.recycling())
    e = mte.Engine(0)
    try:
        pairs = load(e, [Item("bad", log=bad), good])
        assert e.replay()["failed_docs"] >= 1
        assert e.status(pairs[0][0])[0] != 0
        (bri, bci), (ri, ci) = pairs
        R, C = len(ref(good)["rows"]), len(ref(good)["cols"])
        out, vals = e.matrix_cells([(bri, bci, SHAPE), (ri, ci, RECT, 0, 0, R, C), (bri, bci, CELL, 0, 0),
                                    (bri, bci, RECT, 0, 0, 1, 1), (ri, ci, CELL, 2, 0), (bri, ci, SHAPE)])
        assert [int(x["status"]) for x in out] == [DOC_FAILED, OK, DOC_FAILED, DOC_FAILED, OK, DOC_FAILED]
        val = Values(e)
        assert val.rect(vals, out[1], R, C) == ref_grid(good) == good.doc.want_grid
        assert val(out[4]["value"]) == ref_cell(good, 2, 0) and len(vals) == R * C
    finally:
        e.close()


def test_resume_cases():
    """The fragmented and the recycling document cut in the middle and resumed from the oracle's summary
    of the prefix (loaded cells and handle tables): the full grid equals the full replay's oracle grid."""
    cuts = me.cuts()
    items = [Item(f"{n}@{k}", log=log[k:], summary=summ) for n, log, k, summ in cuts]
    e = mte.Engine(0)
    try:
        pairs = load(e, items)
        assert e.replay()["failed_docs"] == 0
        got = full_grids(e, items, pairs)
        for (n, log, k, _), it in zip(cuts, items):
            full = grid(json.loads(me.oracle(log).snapshot_json()))
            assert got[it.name] == full == ref_grid(it), it.name
            assert any(v is not None for row in full for v in row)
        assert e.get_info("downloaded") == 0
    finally:
        e.close()


def test_cache_and_invalidation():
    """A second call builds no table; replay() drops them and the rebuilt ones answer the same; a smaller
    batch loaded into the same engine answers for itself (a stale table would show the first batch's cells
    under the same document indices)."""
    first = interleaved(edge_items(names=("frag300", "recycle24", "writers70", "writers40"), big=False))
    e = mte.Engine(0)
    try:
        pairs = load(e, first)
        assert e.replay()["failed_docs"] == 0
        a = check_full_grids(e, first, pairs)
        built = e.get_info("mx_tables_built")
        assert built == len(first)   # one per matrix, the empty ones included
        assert check_full_grids(e, first, pairs) == a and e.get_info("mx_tables_built") == built
        out, _ = e.matrix_cells([(ri, ci, CELL, 0, 0) for ri, ci in pairs])
        assert e.get_info("mx_tables_built") == built
        assert e.replay()["failed_docs"] == 0
        assert e.get_info("mx_tables_built") == built   # dropped, not yet rebuilt
        assert check_full_grids(e, first, pairs) == a and e.get_info("mx_tables_built") == 2 * built
        small = interleaved(edge_items(names=("recycle24", "writers40"), big=False))[::-1]
        pairs2 = load(e, small)
        assert e.replay()["failed_docs"] == 0
        assert [it.name for it in small] != [it.name for it in first[:len(small)]]
        b = check_full_grids(e, small, pairs2)
        assert e.get_info("mx_tables_built") == 2 * built + len(small)
        assert b["recycle24"] == a["recycle24"] and b["writers40"] == a["writers40"]
        assert e.get_info("downloaded") == 0
    finally:
        e.close()


ROUTES = {"force_hbm": dict(force_hbm=1), "spill": dict(slot_blk_limit=24, pool_limit=48), "retain": dict(retain=1)}


@pytest.mark.parametrize("route", list(ROUTES))
def test_routes_give_the_same_answers(default_answers, route):
    """force_hbm; pool_limit 48 with slot_blk_limit 24 (the DOC_SPILL re-run rewrites cell_h); retain."""
    opts = ROUTES[route]
    items = interleaved(edge_items())
    e = mte.Engine(0)
    try:
        if "slot_blk_limit" in opts:
            e.set_option("slot_blk_limit", opts["slot_blk_limit"])   # (read by the load)
        if "retain" in opts:
            e.retain(True)
        pairs = load(e, items)
        for k in ("force_hbm", "pool_limit"):
            if k in opts:
                e.set_option(k, opts[k])
        assert e.replay()["failed_docs"] == 0
        info = e.run_info()
        if route == "force_hbm":
            assert info["lds_groups"] == 0, info
        if route == "spill":
            assert e.get_info("spilled") > 0, info
        assert check_full_grids(e, items, pairs) == default_answers["grids"]
        assert levels_probe(e, items, pairs) == default_answers["levels"]
        assert e.get_info("downloaded") == 0
    finally:
        e.close()


def test_reader_facade_on_the_spec_cases():
    """SharedMatrixReader over the matrix.spec.ts conflict cases: toArray() equals the spec's literal grid
    (and the oracle's where the spec states none), rowCount / colCount / getCell agree."""
    b = mte.Builder()
    built = {n: build(c) for n, c in CASES.items()}
    pairs = {n: b.add_matrix_log(log, observer="observer") for n, (log, _) in built.items()}
    e = mte.Engine(0)
    try:
        e.load(b.batch())
        assert e.replay()["failed_docs"] == 0
        stated = 0
        for n, (log, expected) in built.items():
            rd = mte.SharedMatrixReader(e, *pairs[n])
            want = grid(oracle_summary(log))
            got = rd.toArray()
            assert got == want, n
            if expected is not None:
                assert got == expected, n
                stated += 1
            assert (rd.rowCount, rd.colCount) == (len(want), len(want[0]) if want else 0), n
            assert rd.getCell(len(want) - 1, len(want[0]) - 1) == want[-1][-1], n
            assert rd.toArray(0, 0, 1, len(want[0])) == want[:1], n
            with pytest.raises(IndexError):
                rd.getCell(len(want), 0)
        assert stated >= 10 and e.get_info("downloaded") == 0
    finally:
        e.close()
