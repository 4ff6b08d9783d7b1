"""GPU: the marker queries (mte_markers) -- findTile and getTextAndMarkers in the observer's current view,
answered on the device from a pass's output rows and their property maps. Every result is compared with
tests/markers.py (the queries restated in Python, pinned to the reference's spec cases by
tests/test_markers_cpu.py) on the oracle's segment table of the same log. No query of these tests may
come back UNSUPPORTED except where a test annotates the tile-label key on purpose (check_markers asserts
it)."""
import ctypes
import random

import numpy as np
import pytest

from fluidframework_amd import mte
from oracle import OracleDoc
from tests import markers
from tests.markers import (BAD_QUERY, DOC_FAILED, NOT_FOUND, OBSERVER, OK, PARAGRAPHS, TILE_AFTER, TILE_BEFORE, TO_END,
                           UNSUPPORTED, Writer, check_markers, text_seg, tile)
from tests.oplog import dumps, ins, msg
from tests.test_gpu_fuzz import random_json_log
from tests.views import rows_of

pytestmark = pytest.mark.gpu

MODES_SOLO = (3, 4)  # DocRes.mode: solo on the LDS engine / on the row engine


def table(log):
    o = OracleDoc(OBSERVER)
    o.apply_json(dumps(log))
    assert o.status()[0] == 0, o.status()
    return rows_of(o)


def load(e, logs):
    b = mte.Builder()
    for log in logs:
        b.add_doc(log, observer=OBSERVER)
    e.load(b.batch())
    return e.replay()


def length(rows):
    return sum(markers.net_len(r) for r in rows)


def every_position(d, rows, label=0):
    """BEFORE and AFTER at every position 0 .. length + 2 of document d, and its paragraphs."""
    q = []
    for p in range(length(rows) + 3):
        q += [(d, TILE_BEFORE, p, 0, label), (d, TILE_AFTER, p, 0, label)]
    return q + [(d, PARAGRAPHS, 0, TO_END, label)]


@pytest.fixture(scope="module")
def engine():
    e = mte.Engine(0)
    yield e
    e.close()


SEAM_LOGS = [markers.seam_log(), markers.seam_log(200, tiles=(0,)), markers.seam_log(64, tiles=(63,)),
             markers.seam_log(65, tiles=()), markers.seam_log(1), []]
_seam = {}


def seam_case():
    if not _seam:
        _seam["tables"] = [table(log) for log in SEAM_LOGS]
        _seam["queries"] = [q for d, rows in enumerate(_seam["tables"]) for q in every_position(d, rows)]
    return _seam["tables"], _seam["queries"]


@pytest.mark.parametrize("route", ["bulk", "solo", "retained"])
def test_seams_on_every_route(route):
    """Tiles on rows 0, 62, 63, 64, 65 and the last row of a 140-row document (and documents whose only tiles
    are two steps apart): both directions at every position, so probes sit on each side of each tile and of
    the 64-row step -- the same answers whichever kernel left the rows."""
    tables, queries = seam_case()
    e = mte.Engine(0)
    try:
        if route == "solo":
            e.set_option("solo_min_ops", 1)
            parts = []
            for d, log in enumerate(SEAM_LOGS):
                load(e, [log])
                mode = e.doc_result(0)["mode"]
                if log:
                    assert e.run_info()["solo"] == 1 and mode in MODES_SOLO, (d, mode, e.run_info())
                parts.append(check_markers(e, [tables[d]], [(0,) + q[1:] for q in queries if q[0] == d], ["EOP"])[0])
                assert e.get_info("downloaded") == 0
            res = np.concatenate(parts)
        else:
            if route == "retained":
                e.retain(True)
                b = mte.Builder()
                ids = [b.open_doc(OBSERVER) for _ in SEAM_LOGS]
                for d, log in zip(ids, SEAM_LOGS):
                    if len(log) > 1:
                        b.append(d, log[: len(log) // 2])
                e.load(b.batch())
                e.replay()
                for d, log in zip(ids, SEAM_LOGS):
                    if log:
                        b.append(d, log[len(log) // 2:])
                e.load(b.batch())
                e.replay()
                assert e.get_info("resumed_docs") + e.get_info("resumed_docs_blk") > 0
            else:
                load(e, SEAM_LOGS)
            modes = [e.doc_result(d)["mode"] for d in range(len(SEAM_LOGS))]
            assert not set(modes) & set(MODES_SOLO), modes
            res, _, _ = check_markers(e, tables, queries, ["EOP"])
            assert e.get_info("downloaded") == 0
        res = res[["status", "row", "pos", "flags", "count"]].tolist()  # (first_piece counts per call)
        if "res" in _seam:
            assert res == _seam["res"]
        _seam["res"] = res
    finally:
        e.close()


def test_pos_equals_length_and_removed_tiles(engine):
    """pos == length with the last row a visible tile, a removed tile still in the table and a text row;
    pos > length in both directions; an empty document; removed tiles in the middle are skipped."""
    a = Writer()  # the last row a visible tile
    a.append("ab"), a.append(tile()), a.append("cd"), a.append(tile())
    b = Writer()  # ... a removed tile (MSN 0: it stays in the table)
    b.append("ab"), b.append(tile()), b.append("cd"), b.append(tile())
    b.remove(5, 6, client="r")
    c = Writer()  # ... a text row
    c.append(tile()), c.append("ab")
    m = Writer()  # removed tiles in the middle, on both sides of a kept one
    for i in range(70):
        m.append(tile() if i % 5 == 0 else "xy")
    for row in (65, 60, 10, 5):  # (from the back: positions hold)
        p = sum(1 if i % 5 == 0 else 2 for i in range(row))
        m.remove(p, p + 1, client="r")
    gone = Writer()  # every row removed
    gone.append(tile()), gone.append("ab")
    gone.remove(0, 3, client="r")
    logs = [a.log, b.log, c.log, m.log, gone.log, []]
    tables = [table(log) for log in logs]
    assert "removedSeq" in tables[1][-1] and sum("removedSeq" in r for r in tables[3]) == 4
    load(engine, logs)
    q = [x for d, rows in enumerate(tables) for x in every_position(d, rows)]
    res, _, _ = check_markers(engine, tables, q, ["EOP"])
    at_len = {d: res[[i for i, x in enumerate(q) if x[:3] == (d, TILE_AFTER, length(tables[d]))][0]] for d in range(6)}
    assert (int(at_len[0]["status"]), int(at_len[0]["row"]), int(at_len[0]["pos"]), int(at_len[0]["flags"])) == (OK, 3, 5, 0)
    assert (int(at_len[1]["status"]), int(at_len[1]["row"]), int(at_len[1]["pos"]), int(at_len[1]["flags"])) == (OK, 3, 5, 1)
    assert int(at_len[2]["status"]) == NOT_FOUND and int(at_len[5]["status"]) == NOT_FOUND
    assert (int(at_len[4]["status"]), int(at_len[4]["flags"])) == (NOT_FOUND, 0)  # the last row there is text
    assert engine.get_info("downloaded") == 0


def test_label_values_and_map_width(engine):
    """The label without the Tile bit, an array of three labels, a string value (its code points), null, a
    number, more than 64 distinct label values in one batch (the bitmap passes one word), and a marker with
    nine properties (the batch takes the wide map record) beside a batch on the narrow one."""
    w = Writer()
    values = [("EOP",), ("H1", "EOP", "Q"), "EQ", "\U0001F600x", None, 7, True, {"EOP": 1}, ("Q",)]
    for v in values:
        w.append(tile(v))
        w.append("t")
    w.append(tile(("EOP",), ref_type=2))  # the label, no Tile bit
    w.append(tile(("EOP",), ref_type=3))  # Tile | NestBegin
    for i in range(80):                   # 80 more distinct values: value ids pass 64 and 96
        w.append(tile((f"L{i}", "EOP") if i % 9 == 0 else (f"L{i}",)))
        w.append("u")
    labels = ["EOP", "H1", "Q", "E", "\U0001F600", "L70", "L79", "7", "nope"]
    narrow = w.log
    wide = Writer()
    wide.append("ab")
    wide.append(tile(("EOP",), **{f"p{i}": i for i in range(8)}))  # nine properties
    wide.append(text_seg("cd", bold="bold"))
    wide.append(tile(("H1",)))
    for logs, words in (([narrow, []], 16), ([narrow, wide.log], None)):
        tables = [table(log) for log in logs]
        load(engine, logs)
        if words:
            assert engine.get_info("map_words") == words
        else:
            assert engine.get_info("map_words") > 16
        q = []
        for d, rows in enumerate(tables):
            L = length(rows)
            for li in range(len(labels)):
                q += [(d, k, p, 0, li) for k in (TILE_BEFORE, TILE_AFTER) for p in (0, 1, L // 3, L // 2, L - 1, L, L + 1) if p >= 0]
                q.append((d, PARAGRAPHS, 0, TO_END, li))
        res, pieces, _ = check_markers(engine, tables, q, labels)
        counts = {li: int(res[[i for i, x in enumerate(q) if x == (0, PARAGRAPHS, 0, TO_END, li)][0]]["count"]) for li in range(len(labels))}
        assert counts == {0: 12, 1: 1, 2: 3, 3: 1, 4: 1, 5: 1, 6: 1, 7: 0, 8: 0}, counts
    assert engine.get_info("downloaded") == 0


def paragraph_log():
    """Every tag transition (the twenty of the table, chained), tag states carried across tiles and across
    the 64-row step, an empty piece between adjacent tiles, a row over 64 units, surrogate pairs split across
    rows, and text behind the last tile."""
    w = Writer()
    combos = {"": (None, None), "b": ("bold", None), "u": (None, "underline"), "bu": ("700", True)}
    # from every state (reached from [] by the path's tag lists), every tag list, then a row that closes all
    for state_path in (["b"], ["u"], ["bu"], ["b", "bu"], []):  # reach [b], [u], [u,b], [b,u], []
        for t in ("", "b", "u", "bu"):
            for s in state_path:
                w.append(text_seg("s", *combos[s]))
            w.append(text_seg("x" + t, *combos[t]))
            w.append(text_seg("r", 0, ""))  # falsy values: closes all
    w.append(tile())
    w.append(tile())  # an empty piece
    w.append(text_seg("bold over a tile", bold=1))
    w.append(tile())
    w.append(text_seg("still bold", bold="yes"))
    while len(w.log) < 126:
        w.append(text_seg("ab", under="u") if len(w.log) >= 120 else "pq")
    for _ in range(6):  # [u] carried across row 127 | 128
        w.append(text_seg("cd", under="u"))
    w.append(tile(("EOP", "H1")))
    w.append("".join(chr(0x400 + k) for k in range(150)))  # a row over 64 units
    w.append("\U0001F600\U0001F601")
    w.insert(w.length - 1, "mid")  # splits the second pair: high | mid | low
    w.insert(w.length - 6, tile(("H1",)))  # ... and a tile inside the first pair
    w.append(tile())
    w.append("dropped text")
    return w.log


def test_paragraphs(engine):
    log = paragraph_log()
    rows = table(log)
    small = [msg("a", 1, 0, ins(0, "hello")), msg("a", 2, 1, ins(5, tile())), msg("a", 3, 2, ins(6, text_seg("w", under=1)))]
    logs = [log] + [small] * 40 + [[]]
    tables = [rows] + [table(small)] * 40 + [[]]
    load(engine, logs)
    L = length(rows)
    starts = [0]
    for r in rows:
        starts.append(starts[-1] + markers.net_len(r))
    q = [(0, PARAGRAPHS, 0, TO_END, 0), (0, PARAGRAPHS, 0, L, 1), (0, PARAGRAPHS, 0, L + 9, 0), (0, PARAGRAPHS, L, L + 1, 0),
         (0, PARAGRAPHS, 7, 7, 0)]
    long_row = next(i for i, r in enumerate(rows) if r["len"] == 150)
    q += [(0, PARAGRAPHS, starts[long_row] + 3, starts[long_row + 1] + 2, 0),   # cut inside a text row at both ends
          (0, PARAGRAPHS, 1, starts[long_row] + 70, 0), (0, PARAGRAPHS, starts[long_row] + 70, TO_END, 1)]
    rng = random.Random(3)
    for _ in range(60):
        a = rng.randint(0, L)
        q.append((0, PARAGRAPHS, a, a + rng.choice([0, 1, 5, 40, 200, 2000]), rng.randint(0, 1)))
    many = [(d, PARAGRAPHS, 0, TO_END, 0) for d in range(1, 42)]  # many documents in one call
    res, pieces, text = check_markers(engine, tables, q + many, ["EOP", "H1"])
    whole = markers.paragraphs(rows, "EOP")
    assert any(p["units"] == [] for p in whole[1:]) and len(whole) == 5 and len(text) > 500
    back, _, _ = check_markers(engine, tables, list(reversed(q + many)), ["EOP", "H1"])
    assert [int(x) for x in back["count"]] == [int(x) for x in reversed(res["count"])]
    # the sizing call, buffers too small, then the real call
    arr = np.array([(0, PARAGRAPHS, 0, TO_END, 0), (1, PARAGRAPHS, 0, TO_END, 0)], dtype=mte.MARK_Q_DTYPE)
    out = np.zeros(2, dtype=mte.MARK_R_DTYPE)
    names = (ctypes.c_char_p * 1)(b"EOP")
    n_p, n_t = ctypes.c_size_t(), ctypes.c_size_t()
    fn = mte.lib().mte_markers
    assert fn(engine._h, arr.ctypes.data, 2, names, 1, out.ctypes.data, None, 0, ctypes.byref(n_p), None, 0, ctypes.byref(n_t)) == 0
    want_t = sum(len(p["units"]) for p in whole) + 5
    assert (n_p.value, n_t.value) == (len(whole) + 1, want_t) and [int(x) for x in out["count"]] == [len(whole), 1]
    pc = np.zeros(n_p.value, dtype=mte.MARK_PIECE_DTYPE)
    tx = np.zeros(n_t.value, dtype=np.uint16)
    for caps in ((n_p.value - 1, n_t.value), (n_p.value, n_t.value - 1)):
        assert fn(engine._h, arr.ctypes.data, 2, names, 1, out.ctypes.data, pc.ctypes.data, caps[0], ctypes.byref(n_p),
                  tx.ctypes.data, caps[1], ctypes.byref(n_t)) == -7
        assert (n_p.value, n_t.value) == (len(whole) + 1, want_t)
    assert fn(engine._h, arr.ctypes.data, 2, names, 1, out.ctypes.data, pc.ctypes.data, n_p.value, ctypes.byref(n_p),
              tx.ctypes.data, n_t.value, ctypes.byref(n_t)) == 0
    assert tx[int(pc[-1]["text_off"]):].tolist() == markers.units("hello") and int(pc[-1]["pos"]) == 5
    assert engine.get_info("downloaded") == 0


def test_refusals(engine):
    """An annotate that sets referenceTileLabels: UNSUPPORTED for both TILE kinds while PARAGRAPHS answers;
    a failed document, a bad label index, pos2 < pos1, an unknown kind and a document out of range."""
    w = Writer()
    w.append("ab"), w.append(tile()), w.append("cd"), w.append(tile(("H1",)))
    w.annotate(2, 3, {markers.TILE_KEY: ["H1"]})
    plain = Writer()
    plain.append("ab"), plain.append(tile()), plain.annotate(0, 3, {"font-weight": "bold"})
    failing = [msg("w", 1, 0, ins(0, "ab")), msg("w", 2, 1, ins(5, "x"))]  # MergeTree insert failed
    logs = [w.log, plain.log, failing]
    load(engine, logs)
    assert engine.status(2)[0] == 1
    rows = table(w.log)
    q = [(0, TILE_BEFORE, 3, 0, 0), (0, TILE_AFTER, 0, 0, 0), (0, PARAGRAPHS, 0, TO_END, 0), (0, PARAGRAPHS, 0, TO_END, 1),
         (1, TILE_BEFORE, 3, 0, 0), (1, PARAGRAPHS, 0, TO_END, 0),
         (2, TILE_BEFORE, 0, 0, 0), (2, PARAGRAPHS, 0, TO_END, 0),
         (0, TILE_BEFORE, 0, 0, 2), (0, PARAGRAPHS, 5, 4, 0), (0, 3, 0, 0, 0), (3, TILE_AFTER, 0, 0, 0)]
    res, pieces, text = engine.markers(q, ["EOP", "H1"])
    assert [int(s) for s in res["status"]] == [UNSUPPORTED, UNSUPPORTED, OK, OK, OK, OK, DOC_FAILED, DOC_FAILED,
                                               BAD_QUERY, BAD_QUERY, BAD_QUERY, BAD_QUERY]
    # PARAGRAPHS reads leaves only: the annotated marker now carries H1
    want = [markers.paragraphs(rows, "EOP"), markers.paragraphs(rows, "H1")]
    assert [int(res[2]["count"]), int(res[3]["count"])] == [len(want[0]), len(want[1])] == [0, 2]
    assert [(int(p["row"]), int(p["pos"])) for p in pieces[:2]] == [(w_["row"], w_["pos"]) for w_ in want[1]]
    assert (int(res[4]["row"]), int(res[4]["pos"])) == (1, 2) and int(res[5]["count"]) == 1
    assert engine.get_info("downloaded") == 0


def test_random_logs_one_call(engine):
    """Random JSON logs (tests/test_gpu_fuzz's generator) with tile markers and the two tag properties added:
    a few hundred queries of every kind and three labels in ONE call."""
    writers = [2, 3, 8, 20]
    logs = [markers.tiled(random_json_log(seed, 300, n_writers=writers[seed % 4], emoji=seed % 2 == 1), seed) for seed in range(8)]
    logs += [markers.tiled(markers_no_msn(log), 50 + i) for i, log in enumerate(logs[:4])]
    tables = [table(log) for log in logs]
    load(engine, logs)
    labels = ["EOP", "H1", "\U0001F600", "E"]
    rng = random.Random(11)
    q = []
    for d, rows in enumerate(tables):
        assert engine.doc_result(d)["status"] == 0 and engine.doc_result(d)["n_segs"] == len(rows)
        L = length(rows)
        for _ in range(30):
            p = rng.randint(0, L + 2)
            q.append((d, rng.choice([TILE_BEFORE, TILE_AFTER]), p, 0, rng.randrange(4)))
        q += [(d, TILE_AFTER, L, 0, li) for li in range(4)]
        q += [(d, PARAGRAPHS, 0, TO_END, li) for li in range(3)]
        for _ in range(6):
            a = rng.randint(0, L)
            q.append((d, PARAGRAPHS, a, a + rng.choice([0, 3, 30, 300, 3000]), rng.randrange(4)))
    rng.shuffle(q)
    res, pieces, text = check_markers(engine, tables, q, labels)
    print("random logs:", len(q), "queries,", len(pieces), "pieces,", len(text), "units,", sum(int(s) == OK for s in res["status"]), "ok")
    assert len(q) > 400 and len(pieces) >= 50 and sum(int(s) == OK for s in res["status"]) >= 250  # (the seeds are fixed: not vacuous)
    assert ord("<") in text.tolist()
    assert engine.get_info("downloaded") == 0


def markers_no_msn(log):
    return [dict(m, minimumSequenceNumber=0) for m in log]


def test_before_a_replay():
    e = mte.Engine(0)
    try:
        with pytest.raises(mte.MteError, match=r"\(-4\)"):  # MTE_E_STATE
            e.markers([(0, TILE_BEFORE, 0, 0, 0)], ["EOP"])
        b = mte.Builder()
        b.add_doc([msg("a", 1, 0, ins(0, "x"))], observer=OBSERVER)
        e.load(b.batch())
        with pytest.raises(mte.MteError, match=r"\(-4\)"):
            e.markers([(0, PARAGRAPHS, 0, TO_END, 0)], ["EOP"])
    finally:
        e.close()


def test_facade():
    """MergeTreeClient.findTile / getTextAndMarkers on the reference's spec cases (client.spec.ts:75-151,
    sharedString.spec.ts:150-182), incrementally."""
    c = mte.MergeTreeClient(observer=OBSERVER)
    try:
        w = Writer()
        for i, (pos, seg) in enumerate([(0, tile(markerId="m0")), (0, "abc d"), (0, tile(markerId="m1")), (7, "ef"),
                                        (8, tile(markerId="m2"))]):
            w.insert(pos, seg)
        for m in w.log:
            c.applyMsg(m)
        assert c.getLength() == 10
        assert c.findTile(5, "EOP")["pos"] == 0 and c.findTile(5, "EOP", False)["pos"] == 6
        assert c.findTile(11, "EOP", False) is None and c.findTile(1, "H1") is None
        got = c.getTextAndMarkers("EOP")
        assert got["parallelText"] == ["", "abc d", "e"]
        assert [m["pos"] for m in got["parallelMarkers"]] == [0, 6, 8]
        assert [m["properties"]["markerId"] for m in got["parallelMarkers"]] == ["m1", "m0", "m2"]
        w.append(text_seg("bold", bold="bold"))
        w.append(tile(("tileLabel",), markerId="tileMarkerId"))
        for m in w.log[-2:]:
            c.applyMsg(m)
        got = c.getTextAndMarkers("tileLabel")
        assert got["parallelText"] == ["abc def<b>bold"] and got["parallelMarkers"][0]["properties"]["markerId"] == "tileMarkerId"
        assert c.findTile(0, "tileLabel", False) == {"pos": 14, "row": got["parallelMarkers"][0]["row"]}
    finally:
        c._engine.close()
