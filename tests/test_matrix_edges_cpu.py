"""The preconditions of tests/matrix_edges.py's documents, on the oracle alone: each builder is on the
intended side of its seam (segment counts, handle-table lengths, recycled handles, undefined sets),
its closed-form expectation equals the oracle's grid / handles / handle tables, and the builder's
record path replays to what the JSON path does. A generator change that weakens a GPU case in
tests/test_gpu_matrix_edges.py fails here first."""
import ctypes
import json

import numpy as np
import pytest

from fluidframework_amd import mte
from oracle import OracleDoc, OracleMatrix
from tests import matrix_edges as me
from tests.oplog import dumps
from tests.test_matrix_spec import get_cell, grid

LDS_ORD, PREFIX_TRIP = 128, 64  # leaf blocks: the LDS plan's block list; one 64-lane trip over it


@pytest.fixture(scope="module")
def docs():
    return {d.name: d for d in me.all_docs()}


def test_closed_forms_equal_the_oracle(docs):
    for d in docs.values():
        assert any(x is not None for x in (d.want_grid, d.want_handles, d.want_tables, d.want_cells)), d.name
        me.check_against_oracle(d)


def test_fragmented_segment_counts(docs):
    """Segments of the final row vector against leaf blocks of 8 slots. These vectors grow by the
    sets' splits, so they are long in pass 2 only (contain / cell_handle over long block lists);
    without their sets they are a handful of segments, which is all pass 1 sees -- the document that
    is long in pass 1 is test_spliced_is_long_before_its_first_set's. By count alone only the largest
    is past a seam (1 367 > 8 x 128); the other two are pinned to the counts whose block peaks (72
    and 61) the GPU test asserts, so a change of fragmentation at equal counts shows there."""
    big, over, under = (docs[f"frag{n}"] for n in me.FRAG_SIZES)
    assert big.facts["row_segments"] == 1367 > me.LEAF_SLOTS * LDS_ORD
    assert over.facts["row_segments"] == 323 and under.facts["row_segments"] == 269
    assert under.facts["row_segments"] < over.facts["row_segments"] < me.LEAF_SLOTS * PREFIX_TRIP
    for d in (big, over, under):
        o = me.oracle(d.log)
        n = int(d.name[4:])
        assert me.n_segments(o.cols) == 3
        # every defined set of a new row allocated a handle and none was freed before the tail: the
        # table is as long as the allocations. The tail's four zamboni steps unlink the removed rows
        # they get to (none in the largest document): those handles are on the free list
        assert d.facts["undefined"] == 5 and d.facts["moved"] > n // 8
        t = me.tables(json.loads(o.snapshot_json()))["rows"]
        assert len(t) == d.facts["row_allocs"] + 1
        assert sum(1 for x in t[1:] if x) == {1400: 0, 350: 3, 300: 5}[n]
        # adjusted != raw: sets behind the 16 removed rows reached rows that are still there
        assert len(d.want_grid) == n - 16
        splices = OracleDoc("obs")
        assert splices.apply_matrix_json(dumps([m for m in d.log if "target" in m["contents"]]), "rows") == 0
        assert me.n_segments(splices) <= 8   # what pass 1 (adjustPosition) walks: one leaf block


@pytest.mark.parametrize("name,n,min_far,moved", [("spliced700", 700, 611, 14), ("spliced560r", 560, 521, 4)])
def test_spliced_is_long_before_its_first_set(docs, name, n, min_far, moved):
    """The row vector adjustPosition sees: n one-row segments from the splices alone, before the
    first set and to the end of the log's splices -- more than 8 x 64, so more than 64 leaf blocks
    whatever their fill -- and every far set's position has more than 512 one-row segments in front
    of it: its prefix sums block summaries past the 64th."""
    d = docs[name]
    f = d.facts
    head = d.log[:f["first_set"]]
    assert all("target" in m["contents"] and m["minimumSequenceNumber"] == 0 for m in head)
    for log in (head, [m for m in d.log[:-4] if "target" in m["contents"]]):
        v = OracleDoc("obs")
        assert v.apply_matrix_json(dumps(log), "rows") == 0
        segs = json.loads(v.segments_json())
        assert len(segs) == n > me.LEAF_SLOTS * PREFIX_TRIP and all(x["len"] == 1 for x in segs)
    assert f["min_far"] == min_far > me.LEAF_SLOTS * PREFIX_TRIP
    assert f["moved"] == moved and f["undefined"] == 4
    assert len(d.want_grid) == n - 20
    far = {v for row in d.want_grid for v in row if isinstance(v, str) and v.startswith("far")}
    assert len(far) == f["moved"]   # every lagging set beyond the hole landed on a row that is still there


def test_handle_levels(docs):
    d = docs["levels4200"]
    o, s = me.check_against_oracle(d)
    t = me.tables(s)
    assert len(t["rows"]) == len(t["cols"]) == 4201 > 4096
    root = json.loads({e["path"]: e["value"] for e in s["entries"]}["cells"]["contents"])[0]
    for b in me.LEVELS:
        for hr, hc in ((b - 1, b - 1), (b - 1, b), (b, b - 1), (b, b)):
            assert get_cell(root, hr, hc) == d.want_cells[(hr, hc)], (hr, hc)
        one_axis = [k for k in d.facts["corner"] if (k[0] >= b) != (k[1] >= b)]
        assert {k[0] >= b for k in one_axis} == {True, False}
    assert me.n_segments(o.rows) > me.LEAF_SLOTS * LDS_ORD and me.n_segments(o.cols) > me.LEAF_SLOTS * LDS_ORD


def test_big_handle_summary():
    """Row handles >= 65 536 through a summary: root index 2 (the Morton key of high halves (1, 0)), a
    table of 65 601 entries, the freed sub-range -- handles 65 534 .. 65 538, straddling the boundary
    -- chained in ascending order, its cells cleared under root index 0 and under index 2. Builder plus
    oracle take well under a second."""
    summary, suffix, want = me.big_handle_summary()
    o = OracleMatrix("obs")
    assert o.load_summary(summary) == 0 and o.apply_json(dumps(suffix)) == 0
    s = json.loads(o.snapshot_json())
    t = me.tables(s)
    assert t["rows"] == want["rows_table"] and len(t["rows"]) == 65601 and t["cols"] == want["cols_table"]
    assert t["rows"][0] == 65538 and t["rows"][65534:65539] == [65601, 65534, 65535, 65536, 65537]
    assert me.blob_cells(s) == want["cells"]
    assert sum(1 for rh, _ in want["cells"] if rh >= 65536) == 3
    before = OracleMatrix("obs")   # the six sets alone: both cells of the range are there to be cleared
    assert before.load_summary(summary) == 0 and before.apply_json(dumps(suffix[:6])) == 0
    cells = me.blob_cells(json.loads(before.snapshot_json()))
    assert cells[(65535, 2)] == "cutlo" and cells[(65536, 3)] == "cuthi"
    assert (65535, 2) not in want["cells"] and (65536, 3) not in want["cells"]
    root = json.loads({e["path"]: e["value"] for e in s["entries"]}["cells"]["contents"])[0]
    assert len(root) == 3 and root[1] is None and root[2] is not None   # root_len 3: index 2 = row half 1
    assert get_cell(root, 65540, 2) == "hi0" and get_cell(root, 65532, 1) == "lo"
    assert len(me.handles(s)["rows"]) == want["rows"] == 65595


def test_recycling_is_lifo(docs):
    d = docs["recycle24"]
    n, f = d.facts["n"], d.facts
    # coalesced multi-handle runs stand in the oracle's segment table before the remove: zamboni
    # merges inside a leaf block only, so handles 1 .. n are six runs of 3 to 5, in ascending order
    segs = json.loads(me.oracle(d.log[:f["run_at"]]).rows.segments_json())
    runs = [(x["start"], x["len"]) for x in segs if x["start"] != me.UNALLOC]
    assert runs == [(1, 3), (4, 4), (8, 4), (12, 4), (16, 4), (20, 5)] and runs[-1][0] + runs[-1][1] == n + 1, segs
    # after the UNLINK: the whole free list, head n, handle h linking to h - 1, handle 1 to the top
    t = me.tables(json.loads(me.oracle(d.log[:f["cut"]]).snapshot_json()))["rows"]
    assert t == f["freed_table"] == [n, n + 1] + list(range(1, n))
    # n + 1 allocations: n, n - 1, .., 1, then the never-used n + 1; the concurrent set took none
    assert f["realloc"] == list(range(n, 0, -1)) + [n + 1] and f["undefined"] == 1
    o, s = me.check_against_oracle(d)
    assert me.tables(s)["rows"] == [n + 2] + [0] * (n + 1)
    assert me.handles(s)["rows"] == [None] + list(range(n, 0, -1)) + [n + 1, None, None]
    g = grid(s)
    root = json.loads({e["path"]: e["value"] for e in s["entries"]}["cells"]["contents"])[0]
    for i in range(n + 1):
        # even rows set the old key (handle, col handle 1) again: the new value; odd rows did not: null
        assert g[1 + i] == ([f"new{i}", None] if i % 2 == 0 else [None, f"new{i}"])
    assert root[0][0][0][0] is not None and get_cell(root, n - 1, 1) is None   # cleared in place: the tile stays


def test_many_writers_bands(docs):
    for name, nw, slots in (("writers70", 70, (6, 41, 69)), ("writers40", 40, (6, 34, 39))):
        d = docs[name]
        seen = []
        for m in d.log:
            if m["clientId"] not in seen:
                seen.append(m["clientId"])
            if len(seen) < nw:
                assert m["minimumSequenceNumber"] == 0   # nobody's short id is given up
        assert len(seen) == nw
        # short ids follow first appearance, the observer holding 0
        assert tuple(seen.index(w) + 1 for w in d.facts["bands"]) == slots
        assert d.facts["undefined"] == 14 and d.facts["defined"] == 25
        me.check_against_oracle(d)
        # before the tail unlinks them: rows removed by the first band with the other two in the
        # overlap set, by the second with the third, and by the third alone
        segs = json.loads(me.oracle(d.log[:-4]).rows.segments_json())
        b = d.facts["bands"]
        got = {(x["removedClient"], tuple(x["overlap"])) for x in segs if "removedSeq" in x}
        assert got == {(b[0], ()), (b[0], (b[1],)), (b[0], (b[1], b[2])), (b[1], (b[2],)), (b[2], ())}, got
        if nw == 70:
            assert max(slots) >= 64


def test_cuts_resume_to_the_full_replay():
    for name, log, k, summ in me.cuts():
        assert 0 < k < len(log)
        r = OracleMatrix("obs")
        assert r.load_summary(summ) == 0 and r.apply_json(dumps(log[k:])) == 0
        assert grid(json.loads(r.snapshot_json())) == grid(json.loads(me.oracle(log).snapshot_json())), name
        assert any("target" not in m["contents"] for m in log[k:]), name   # the suffix still sets cells


def test_builder_records_agree_with_json_path(docs):
    """As test_builder_matrix_cell_records: one MTE_OP_CELL record per set in both documents, in set
    order, with the message's seq and position; and the vectors' splices replay (records, no cells) to
    the oracle's vector-only JSON path."""
    for d in docs.values():
        sets = [x for x in d.log if "target" not in x["contents"]]
        b = mte.Builder()
        ri, ci = b.add_matrix_log(d.log, observer="obs")
        batch = b.batch()
        ops = mte.batch_ops(batch)
        offs = np.ctypeslib.as_array(batch.doc_op_offsets, shape=(3,))
        for doc, key in ((ri, "row"), (ci, "col")):
            cell = ops[offs[doc]:offs[doc + 1]]
            cell = cell[cell["type"] == 10]
            assert len(cell) == len(sets), d.name
            assert list(cell["seq"]) == [x["sequenceNumber"] for x in sets]
            assert list(cell["ref_seq"]) == [x["referenceSequenceNumber"] for x in sets]
            assert list(cell["pos1"]) == [x["contents"][key] for x in sets]
        splices = [x for x in d.log if "target" in x["contents"]]
        for doc, tgt in ((ri, "rows"), (ci, "cols")):
            b2 = mte.Builder()
            r2, c2 = b2.add_matrix_log(splices, observer="obs")
            rec, o = OracleDoc("obs"), OracleDoc("obs")
            rec.apply_batch(ctypes.addressof(b2.batch()), r2 if tgt == "rows" else c2)
            assert o.apply_matrix_json(dumps(splices), tgt) == 0
            assert rec.status()[0] == 0 and rec.segments_json() == o.segments_json(), (d.name, tgt)
