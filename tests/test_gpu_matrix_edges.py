"""SharedMatrix cell replay on the GPU at its seams and on every route of the pass.

The documents are tests/matrix_edges.py's (each one's edge is pinned on the oracle alone by
tests/test_matrix_edges_cpu.py): row vectors that the sets' splits grow to 269 / 323 / 1 367 segments
(pass 2's contain / cell_handle over block lists either side of 64 and past the LDS plan's 128 leaf
blocks, where pass 2 leaves the plan in the middle of a run of cell ops while pass 1 -- which never
splits -- walked one block), row vectors of 700 and 560 segments from their splices alone (pass 1's
cell_adjust sums block summaries past the 64th: obs_prefix's second trip), handles past 16 / 256 /
4 096 on both axes and past 65 536 through a summary, an engineered LIFO recycling, 70 and 40
writers with overlapping removes from every band of the removers words. Every check compares both
vectors' segment tables and SnapshotV1 trees and the whole matrix summary with the oracle's, and the
cells with the builders' closed forms; every route asserts from run_info / doc_result that it was
taken and that its summaries equal the default route's byte for byte."""
import json

import pytest

from fluidframework_amd import mte
from oracle import OracleDoc, OracleMatrix
from tests import matrix_edges as me
from tests.oplog import dumps
from tests.test_matrix_spec import grid

pytestmark = pytest.mark.gpu

MODE_LDS, MODE_HBM, MODE_CONTINUED = 0, 1, 2   # DocRes.mode (engine.hpp finish)
MODES_SOLO = (3, 4)
LDS_ORD = 128  # WaveRegion::ord (engine_types.hpp): leaf blocks of a document in the LDS plan

_DOCS, _WANT = {}, {}


def docs():
    if not _DOCS:
        for d in me.all_docs():
            _DOCS[d.name] = d
    return _DOCS


class Item:
    """One matrix of a batch: a log, or a summary and its suffix."""

    def __init__(self, name, log=None, summary=None, doc=None):
        self.name, self.log, self.summary, self.doc = name, log, summary, doc

    def add(self, b):
        if self.summary is not None:
            return b.add_matrix_from_summary(self.summary, self.log, observer="obs")
        return b.add_matrix_log(self.log, observer="obs")

    def want(self):
        """The oracle's segment tables, vector snapshots and matrix summary (computed once)."""
        if self.name not in _WANT:
            o = OracleMatrix("obs")
            if self.summary is not None:
                assert o.load_summary(self.summary) == 0
            assert o.apply_json(dumps(self.log)) == 0, self.name
            _WANT[self.name] = {"rows": (o.rows.segments_json(), o.rows.snapshot_json()),
                                "cols": (o.cols.segments_json(), o.cols.snapshot_json()),
                                "tree": json.loads(o.snapshot_json())}
        return _WANT[self.name]


def empty(i):
    return Item(f"empty{i}", log=[])


def big_item():
    summary, suffix, want = me.big_handle_summary()
    it = Item("big65600", log=suffix, summary=summary)
    it.big = want
    return it


def edge_items(names=None, big=True):
    out = [Item(n, log=d.log, doc=d) for n, d in docs().items() if names is None or n in names]
    if big:
        out.append(big_item())
    return out


def interleaved(items):
    """The matrices with an empty one after every second and at both ends."""
    out = [empty(0)]
    for i, it in enumerate(items):
        out.append(it)
        if i % 2:
            out.append(empty(len(out)))
    out.append(empty(len(out)))
    return out


def load(e, items):
    b = mte.Builder()
    pairs = [it.add(b) for it in items]
    e.load(b.batch())
    return pairs


def check(e, items, pairs, same_as=None):
    """Every matrix against the oracle and its closed forms; returns {name: summary bytes}. same_as:
    another route's bytes, which these must equal."""
    out = {}
    for it, (ri, ci) in zip(items, pairs):
        w = it.want()
        for d, axis in ((ri, "rows"), (ci, "cols")):
            assert e.status(d)[0] == 0, (it.name, axis, e.status(d), e.doc_result(d))
            assert e.segments_json(d) == w[axis][0], (it.name, axis)
            assert e.snapshot_json(d) == w[axis][1], (it.name, axis)
        raw = e.snapshot_matrix(ri, ci)
        got = json.loads(raw)
        assert got == w["tree"], it.name
        d = it.doc
        if d is not None:
            if d.want_grid is not None:
                assert grid(got) == d.want_grid, it.name
            if d.want_handles is not None:
                assert me.handles(got) == d.want_handles, it.name
            if d.want_tables is not None:
                assert me.tables(got) == d.want_tables, it.name
            if d.want_cells is not None:
                assert me.blob_cells(got) == d.want_cells, it.name
        if getattr(it, "big", None):
            t = me.tables(got)
            assert t["rows"] == it.big["rows_table"] and t["cols"] == it.big["cols_table"]
            assert me.blob_cells(got) == it.big["cells"]
            assert len(me.handles(got)["rows"]) == it.big["rows"]
        if same_as is not None and it.name in same_as:
            assert raw == same_as[it.name], it.name
        out[it.name] = raw
    return out


def cell_docs(items, pairs):
    """(name, axis, doc index) of every vector that carries cell records."""
    return [(it.name, a, d) for it, p in zip(items, pairs) if it.log for a, d in zip(("rows", "cols"), p)]


def modes(e, items, pairs):
    return {(n, a): e.doc_result(d)["mode"] for n, a, d in cell_docs(items, pairs)}


@pytest.fixture(scope="module")
def default_bytes():
    """The default route over the whole edge batch, forward: every later route compares with it."""
    items = interleaved(edge_items())
    e = mte.Engine(0)
    try:
        pairs = load(e, items)
        st = e.replay()
        assert st["failed_docs"] == 0, st
        out = check(e, items, pairs)
        info, md = e.run_info(), modes(e, items, pairs)
        res = {it.name: e.doc_result(p[0]) for it, p in zip(items, pairs)}
        w70 = pairs[[it.name for it in items].index("writers70")][0]
        slot70 = e.client_slot(w70, docs()["writers70"].facts["bands"][-1])
    finally:
        e.close()
    return {"bytes": out, "info": info, "modes": md, "res": res, "slot70": slot70}


def test_default_route_seams(default_bytes):
    """Default options. The 1 367-segment row vector passes the LDS plan's 128 block summaries
    (WaveRegion::ord) in pass 2 and leaves the plan; the two smaller ones peak either side of 64 leaf
    blocks (pass 2's contain over one and over two 64-block trips) and stay LDS-resident. The spliced
    vectors are 700 and 560 segments before their first set, so pass 1 too walks more than 64 leaf
    blocks and cell_adjust's prefix (obs_prefix) takes its second trip: HBM-resident in the first (it
    has left the plan by then), LDS-resident in the second. No cell document runs solo; a writer
    of the 70-writer document holds a short id >= 64 in the rows vector."""
    res, md, info = default_bytes["res"], default_bytes["modes"], default_bytes["info"]
    big, over, under = (f"frag{n}" for n in me.FRAG_SIZES)
    assert res[big]["max_lb"] > LDS_ORD and res[big]["mode"] in (MODE_HBM, MODE_CONTINUED), res[big]
    assert res[big]["mode"] != MODE_CONTINUED or info["continued"] > 0
    # (a document can leave the plan below 128 blocks too -- its heap or interior nodes fill first: the
    # fragmented vectors of 118 and more did, those up to 100 did not -- so only the sides of 64 are
    # asserted for the smaller two, and that both replayed LDS-resident to the end)
    assert 64 < res[over]["max_lb"] <= LDS_ORD and res[over]["mode"] == MODE_LDS, res[over]
    assert res[under]["max_lb"] < 64 and res[under]["mode"] == MODE_LDS, res[under]
    # (n segments of which none settles before the tail: at least n / 8 blocks, in either pass; the
    # sets split nothing, so the smaller one's pass 1 is as LDS-resident as the pass that reports)
    assert res["spliced700"]["max_lb"] > LDS_ORD and res["spliced700"]["mode"] == MODE_CONTINUED, res["spliced700"]
    assert 64 < res["spliced560r"]["max_lb"] <= LDS_ORD and res["spliced560r"]["mode"] == MODE_LDS, res["spliced560r"]
    assert info["solo"] == 0 and not any(m in MODES_SOLO for m in md.values()), md
    assert default_bytes["slot70"] >= 64


def test_reversed_batch(default_bytes):
    items = interleaved(edge_items()[::-1])
    e = mte.Engine(0)
    try:
        pairs = load(e, items)
        assert e.replay()["failed_docs"] == 0
        check(e, items, pairs, same_as=default_bytes["bytes"])
    finally:
        e.close()


def test_route_force_hbm(default_bytes):
    """force_hbm: every cell document is replayed HBM-resident from its first op (mode 1)."""
    items = interleaved(edge_items())
    e = mte.Engine(0)
    try:
        pairs = load(e, items)
        e.set_option("force_hbm", 1)
        assert e.replay()["failed_docs"] == 0
        info, md = e.run_info(), modes(e, items, pairs)
        assert info["lds_groups"] == 0 and set(md.values()) == {MODE_HBM}, (info, md)
        check(e, items, pairs, same_as=default_bytes["bytes"])
    finally:
        e.close()


# pool_limit: LDS leaf blocks usable per CU (400 by default). This batch has fewer documents than the
# device has CUs, so each has a CU's pool to itself and a shrunken pool alone never fails an op half
# way: tried on an MI355X, pool_limit 96 / 48 / 40 / 24 / 16 gave spilled 0 at every value. Without a
# limit the vectors that outgrow the LDS plan anyway continue HBM-resident (the 1 367-segment one, the
# 700-row spliced one and both 4 200-handle ones); at 48 every vector of more than 48 leaf blocks does:
# the 323- and the 269-segment ones (72 and 61 blocks) and the 560-row spliced one (111), all
# LDS-resident by default. The host's DOC_SPILL re-run is reached through the slot a document continues
# into: with slot_blk_limit 24 as well, the same documents outgrow their slot in the middle of the pass
# (spilled = what continued before, continued 0) and are re-run from ht_reset, rewriting cell_h.
SHRUNK = {"continue": (48, 0), "spill": (48, 24)}   # (pool_limit, slot_blk_limit)


@pytest.mark.parametrize("how", list(SHRUNK))
def test_route_shrunken_pool(default_bytes, how):
    pool, slot = SHRUNK[how]
    items = interleaved(edge_items())
    under = f"frag{me.FRAG_SIZES[-1]}"
    assert default_bytes["modes"][(under, "rows")] == MODE_LDS
    e = mte.Engine(0)
    try:
        e.set_option("slot_blk_limit", slot)   # (read by the load)
        pairs = load(e, items)
        e.set_option("pool_limit", pool)
        assert e.replay()["failed_docs"] == 0
        info, md = e.run_info(), modes(e, items, pairs)
        if how == "continue":
            assert info["continued"] > default_bytes["info"]["continued"] and info["spilled"] == 0, info
            assert md[(under, "rows")] == MODE_CONTINUED, md
        else:
            assert e.get_info("spilled") > 0 and info["hbm_ms"] > 0, info
            assert md[(under, "rows")] != MODE_LDS, md   # re-run by the host, HBM-resident
        check(e, items, pairs, same_as=default_bytes["bytes"])
    finally:
        e.close()


def test_route_slot_overflow(default_bytes):
    """HBM slots of 8 leaf blocks (slot_blk_limit, read by the load) under force_hbm: the long cell
    documents outgrow their slot and the host re-runs them with worst-case capacities."""
    items = interleaved(edge_items())
    e = mte.Engine(0)
    try:
        e.set_option("slot_blk_limit", 8)
        pairs = load(e, items)
        e.set_option("force_hbm", 1)
        assert e.replay()["failed_docs"] == 0
        info = e.run_info()
        assert info["spilled"] > 0 and info["hbm_ms"] > 0, info
        check(e, items, pairs, same_as=default_bytes["bytes"])
    finally:
        e.close()


def test_replay_twice_then_a_smaller_batch(default_bytes):
    """replay() twice on one load gives identical bytes; a smaller matrix batch loaded into the same
    engine afterwards (the handle-table and cell buffers are reused, not reallocated) shows nothing of
    the first one."""
    items = interleaved(edge_items())
    e = mte.Engine(0)
    try:
        pairs = load(e, items)
        assert e.replay()["failed_docs"] == 0
        first = check(e, items, pairs, same_as=default_bytes["bytes"])
        assert e.replay()["failed_docs"] == 0
        assert check(e, items, pairs) == first
        small = interleaved(edge_items(names=("recycle24", "writers40"), big=False))[::-1]
        pairs = load(e, small)
        assert e.replay()["failed_docs"] == 0
        check(e, small, pairs, same_as=default_bytes["bytes"])
    finally:
        e.close()


def test_retain_leaves_a_matrix_batch_unchanged(default_bytes):
    items = interleaved(edge_items())
    e = mte.Engine(0)
    try:
        e.retain(True)
        pairs = load(e, items)
        assert e.replay()["failed_docs"] == 0
        check(e, items, pairs, same_as=default_bytes["bytes"])
        pairs = load(e, items)   # the same logs again: nothing of a cell batch may be resumed wrongly
        assert e.replay()["failed_docs"] == 0
        check(e, items, pairs, same_as=default_bytes["bytes"])
    finally:
        e.close()


def text_logs():
    from tests.test_gpu_fuzz import random_json_log

    short = [random_json_log(4100 + i, 300, n_writers=w, newline=False, emoji=True) for i, w in enumerate((3, 8, 20, 40, 8))]
    long_ = random_json_log(4200, 7000, n_writers=8, newline=False, emoji=True)
    return short, long_


def check_text(e, d, log):
    o = OracleDoc("obs")
    o.apply_json(dumps(log))
    assert e.status(d)[0] == o.status()[0] == 0, (d, e.status(d), o.status())
    assert e.segments_json(d) == o.segments_json(), d
    assert e.snapshot_json(d) == o.snapshot_json(), d


def test_mixed_batch_solo_text_beside_cells(default_bytes):
    """The edge matrices beside SharedString documents (random JSON logs with props, markers, emoji).
    One SharedString is solo-eligible (the longest document, >= 8 x the batch mean, solo_min_ops 1): it
    runs on k_solo in the final pass while pass 1 -- the cell documents alone -- runs no solo
    workgroup and no cell document is ever a solo one. Everything is bit-exact."""
    short, long_ = text_logs()
    # (without the 65 600-handle summary: its 65 601 table records would make it the longest document)
    items = interleaved(edge_items(big=False)) + [empty(100 + i) for i in range(12)]
    b = mte.Builder()
    pairs, tdocs = [], []
    for i, it in enumerate(items):
        pairs.append(it.add(b))
        if i < len(short):
            b.add_doc(short[i], observer="obs")
            tdocs.append((b.n_docs() - 1, short[i]))
    b.add_doc(long_, observer="obs")
    long_doc = b.n_docs() - 1
    e = mte.Engine(0)
    try:
        e.set_option("solo_min_ops", 1)
        e.load(b.batch())
        assert e.replay()["failed_docs"] == 0
        info, md = e.run_info(), modes(e, items, pairs)
        assert info["solo"] == 1 and e.doc_result(long_doc)["mode"] in MODES_SOLO, (info, e.doc_result(long_doc))
        assert not any(m in MODES_SOLO for m in md.values()), md
        check(e, items, pairs, same_as=default_bytes["bytes"])
        for d, log in tdocs + [(long_doc, long_)]:
            check_text(e, d, log)
    finally:
        e.close()


def test_fresh_engine_solo_eligible_cell_vector(default_bytes):
    """One long cell vector (the 1 367-segment one: ~700 records against a mean of ~30) beside many
    short matrices on a fresh engine with solo_min_ops 1: it is not counted solo and it is exact."""
    items = [empty(i) for i in range(20)] + edge_items(names=(f"frag{me.FRAG_SIZES[0]}",), big=False) + \
        edge_items(names=("recycle24",), big=False) + [empty(50 + i) for i in range(20)]
    e = mte.Engine(0)
    try:
        e.set_option("solo_min_ops", 1)
        pairs = load(e, items)
        # the load's own slot plan already knows this batch's cell documents (it used to ask the
        # previous load's set, empty on a fresh engine, and planned a solo slot for the vector)
        assert e.get_info("solo_planned") == 0
        assert e.replay()["failed_docs"] == 0
        info, md = e.run_info(), modes(e, items, pairs)
        assert info["solo"] == 0 and not any(m in MODES_SOLO for m in md.values()), (info, md)
        check(e, items, pairs, same_as=default_bytes["bytes"])
    finally:
        e.close()


def test_reused_engine_keeps_the_text_batch_solo_route():
    """A lean text batch whose longest document has the index of a cell document of the matrix batch
    loaded before it: the solo count equals a fresh engine's, and the results are the same."""
    import numpy as np

    counts = [200] * 48
    counts[1] = 30000   # document 1: the first matrix's cols vector in the batch before
    gen = mte.Engine(0)
    a = mte.Engine(0)
    fresh = mte.Engine(0)
    try:
        gen.generate(2, len(counts), 0, n_clients=8, seed=77, ops_per_doc=counts)
        batch = gen.export_batch()
        items = edge_items(names=("recycle24", "writers40", f"frag{me.FRAG_SIZES[-1]}"), big=False)
        pairs = load(a, items)
        assert a.replay()["failed_docs"] == 0 and 1 in [d for _, _, d in cell_docs(items, pairs)]
        out = []
        for e in (a, fresh):
            e.set_option("solo_min_ops", 1000)
            e.load(batch)
            assert e.get_info("solo_planned") == 1   # (0 on the reused engine while the stale set answered)
            assert e.replay()["failed_docs"] == 0
            out.append((e.run_info()["solo"], e.doc_result(1)["mode"], e.summaries()))
        assert out[0][0] == out[1][0] == 1 and out[0][1] == out[1][1] and out[0][1] in MODES_SOLO, [o[:2] for o in out]
        assert np.array_equal(out[0][2]["checksum"], out[1][2]["checksum"])
    finally:
        for e in (gen, a, fresh):
            e.close()


@pytest.mark.parametrize("limit", [0, SHRUNK["continue"][0]])
def test_resume_cases(limit):
    """The fragmented and the recycling document cut in the middle: the oracle's summary of the prefix
    plus the suffix, on the default route and with a shrunken pool. The resumed summary equals the
    oracle's resumed one and shows the cells of the full replay."""
    cuts = me.cuts()
    items = [Item(f"{n}@{k}", log=log[k:], summary=summ) for n, log, k, summ in cuts]
    e = mte.Engine(0)
    try:
        pairs = load(e, items)
        e.set_option("pool_limit", limit)
        assert e.replay()["failed_docs"] == 0
        assert not limit or e.run_info()["continued"] > 0   # (the resumed 269-segment vector leaves the pool)
        got = check(e, items, pairs)
        for (n, log, k, _), it in zip(cuts, items):
            full = json.loads(me.oracle(log).snapshot_json())
            assert grid(json.loads(got[it.name])) == grid(full), it.name
    finally:
        e.close()
