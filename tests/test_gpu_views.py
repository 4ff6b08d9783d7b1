"""GPU: the view queries (mte_views, mte_client_slot, mte_view_props) -- length, position and text as any
client saw them, answered on the device from a pass's output rows. Every result is compared with
tests/views.py (the queries restated in Python, pinned to the oracle by tests/test_views_cpu.py) on the
oracle's segment table of the same log."""
import ctypes
import random

import numpy as np
import pytest

from fluidframework_amd import mte
from oracle import OracleDoc
from tests import views
from tests.oplog import dumps, ins, msg, rem
from tests.test_gpu_fuzz import random_json_log
from tests.test_many_clients import overlap_log
from tests.views import LENGTH, LOCATE, OBSERVER, TEXT

pytestmark = pytest.mark.gpu

MODES_SOLO = (3, 4)  # DocRes.mode: solo on the LDS engine / on the row engine


def table(log):
    o = OracleDoc(OBSERVER)
    o.apply_json(dumps(log))
    assert o.status()[0] == 0, o.status()
    return views.rows_of(o)


def load(e, logs):
    b = mte.Builder()
    for log in logs:
        b.add_doc(log, observer=OBSERVER)
    e.load(b.batch())
    return e.replay()


def as_text(u):
    return np.asarray(u, dtype=np.uint16).tobytes().decode("utf-16-le", "surrogatepass")


def check_no_download(e, tables):
    """The queries made no whole-pool download; the old read still works, and makes it."""
    assert e.get_info("downloaded") == 0
    for d, rows in enumerate(tables):
        assert e.text(d) == as_text(views.text(rows, 0, OBSERVER))
    assert e.get_info("downloaded") == 1


@pytest.fixture(scope="module")
def engine():
    e = mte.Engine(0)
    yield e
    e.close()


SEAM_LOGS = [views.seam_log(n) for n in views.SEAM_SIZES]
_seam = {}


def seam_case():
    if not _seam:
        _seam["tables"] = [table(log) for log in SEAM_LOGS]
        _seam["queries"] = [q for d, log in enumerate(SEAM_LOGS) for q in views.seam_queries(d, _seam["tables"][d], log)]
    return _seam["tables"], _seam["queries"]


@pytest.mark.parametrize("route", ["bulk", "solo", "retained"])
def test_seams_on_every_route(route):
    """Documents of 0 .. 200 rows with rows of length 0 on both sides of each 64-row step: LENGTH and
    LOCATE at every position of every view, the same answers whichever kernel left the rows."""
    tables, queries = seam_case()
    e = mte.Engine(0)
    try:
        if route == "solo":
            e.set_option("solo_min_ops", 1)
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
        elif route == "bulk":
            load(e, SEAM_LOGS)
        if route == "solo":  # a document is a solo one only alone in its batch (or far longer than the rest)
            parts = []
            for d, log in enumerate(SEAM_LOGS):
                load(e, [log])
                mode = e.doc_result(0)["mode"]
                print(route, "rows", len(tables[d]), "mode", mode)
                if log:
                    assert e.run_info()["solo"] == 1 and mode in MODES_SOLO, (d, mode, e.run_info())
                parts.append(views.check_views(e, [tables[d]], [(0,) + q[1:] for q in queries if q[0] == d])[0])
                check_no_download(e, [tables[d]])
            res = np.concatenate(parts)
        else:
            modes = [e.doc_result(d)["mode"] for d in range(len(SEAM_LOGS))]
            print(route, "modes", modes)
            assert not set(modes) & set(MODES_SOLO), modes
            res, _ = views.check_views(e, tables, queries)
            check_no_download(e, tables)
        if "res" in _seam:
            assert res.tobytes() == _seam["res"].tobytes()
        _seam["res"] = res
    finally:
        e.close()


def test_overlap_words(engine):
    """99 concurrent removers, slots 64..127 in use: the views of removers on both sides of the overlap
    words' seams, and of a client that removed nothing."""
    log = overlap_log(100)
    rows = table(log)
    load(engine, [log])
    who = {s: f"w{s - 1}" for s in (1, 31, 32, 63, 64, 65, 100)}  # short id -> long id (first appearance + 1)
    for s, name in who.items():
        assert engine.client_slot(0, name) == s
    assert engine.client_slot(0, "nobody") == views.NO_CLIENT
    q = []
    for name in list(who.values()) + [None]:
        for ref in (1, len(log)):
            L = views.length(rows, ref, name)
            q += [(0, ref, name, LENGTH, 0, 0), (0, ref, name, TEXT, 0, L), (0, ref, name, TEXT, 1, L + 9)]
            q += [(0, ref, name, LOCATE, p, 0) for p in range(L + 1)]
    q.append((0, 0, OBSERVER, LENGTH, 0, 0))
    views.check_views(engine, [rows], q)
    # the overlap bit alone hides the range for a later remover at refSeq 1: its view is shorter than
    # that of a client without a slot
    assert views.length(rows, 1, "w70") < views.length(rows, 1, None)
    check_no_download(engine, [rows])


def test_random_logs_one_call(engine):
    """Twelve random logs with MSN 0 and the same twelve with their own MSN in one batch: 200 random
    queries of each kind per document, all in ONE call; one query below each window."""
    writers = [2, 3, 8, 20, 40, 70]
    own = [random_json_log(seed, 400, n_writers=writers[seed % 6], emoji=False) for seed in range(12)]
    logs = [views.no_msn(log) for log in own] + own
    tables = [table(log) for log in logs]
    load(engine, logs)
    rng = random.Random(7)
    q, below = [], []
    for d, (log, rows) in enumerate(zip(logs, tables)):
        r = engine.doc_result(d)
        assert r["status"] == 0 and r["n_segs"] == len(rows)
        names = sorted({m["clientId"] for m in log}) + [OBSERVER, None]
        for kind in (LENGTH, LOCATE, TEXT):
            for _ in range(200):
                c, ref = rng.choice(names), rng.randint(r["min_seq"], r["cur_seq"])
                p1 = rng.randint(0, 700)
                q.append((d, ref, c, kind, p1, p1 + rng.choice([0, 1, 5, 40, 2000])))
        if r["min_seq"] > 0:
            below.append((d, r["min_seq"] - 1, 1, LENGTH, 0, 0))
    assert len(below) >= 6
    views.check_views(engine, tables, q)
    res, _ = engine.views(below)
    assert [int(s) for s in res["status"]] == [views.OUT_OF_WINDOW] * len(below)
    # the observer has no window
    res, _ = engine.views([(d, ref, 0, k, a, b) for d, ref, _, k, a, b in below])
    assert [int(s) for s in res["status"]] == [views.OK] * len(below)
    check_no_download(engine, tables)


def text_log():
    """Rows of 1, 31, 32, 33, 64, 65 and 300 units and markers, 80 rows (MSN 0: none merges), a few removed
    by other clients; the rows' units differ, so a shifted copy shows."""
    lens = [1, 31, 32, 33, 64, 65, 300]
    out, pos = [], 0
    for i in range(80):
        if i % 11 == 5:
            seg, n = {"marker": {"refType": 1}}, 1
        else:
            n = lens[i % 7]
            seg = "".join(chr(0x100 + (i * 37 + k) % 0x700) for k in range(n))
        out.append(msg(f"w{i % 3}", i + 1, i, ins(pos, seg), 0))
        pos += n
    seq = 80
    for k, (a, b) in enumerate([(pos - 40, pos - 10), (700, 1100), (30, 34)]):
        seq += 1
        out.append(msg(f"r{k}", seq, seq - 1, rem(a, b), 0))
    return out


def test_text_ranges(engine):
    log = text_log()
    rows = table(log)
    load(engine, [log, []])
    assert len(rows) >= 80 and {r["len"] for r in rows} >= {1, 31, 32, 33, 64, 65, 300}
    starts = [0]
    for r in rows:
        starts.append(starts[-1] + r["len"])  # (row boundaries of the view that sees every row)
    q = []
    for ref, c in [(0, OBSERVER), (80, None), (80, "r1"), (len(log), None), (len(log), "w1"), (40, "w2"), (81, "r0")]:
        L = views.length(rows, ref, c)
        q += [(0, ref, c, TEXT, 0, L), (0, ref, c, TEXT, 0, views.NO_CLIENT), (0, ref, c, TEXT, L, L + 3),
              (0, ref, c, TEXT, L + 1, L + 3), (0, ref, c, TEXT, 7, 7), (0, ref, c, TEXT, max(L - 5, 0), L + 50)]
        for a in (0, 1, 31, 32, 33, 64, 65, 300):
            q += [(0, ref, c, TEXT, s + da, s + a + db) for s in starts[:70:3] for da, db in ((0, 0), (1, 1), (0, 1), (3, -1))
                  if da <= a + db]
        q += [(0, ref, c, TEXT, starts[60], starts[70]), (0, ref, c, TEXT, starts[63] + 1, starts[66] - 1)]  # across row 64
        m = next(i for i, r in enumerate(rows) if r["kind"] == "M")
        q += [(0, ref, c, TEXT, starts[m] - 2, starts[m] + 3), (0, ref, c, TEXT, starts[m], starts[m] + 1)]   # over a marker
    q += [(1, 0, OBSERVER, TEXT, 0, 10), (1, 0, OBSERVER, LENGTH, 0, 0), (1, 0, OBSERVER, LOCATE, 0, 0)]  # an empty document
    res, txt = views.check_views(engine, [rows, []], q)
    assert len(txt) > 10000
    # no client's view at r is the document after the messages up to r (a fresh oracle)
    for r in range(0, len(log) + 1, 9):
        o = OracleDoc(OBSERVER)
        o.apply_json(dumps([m for m in log if m["sequenceNumber"] <= r]))
        got, t = engine.views([(0, r, views.NO_CLIENT, TEXT, 0, views.NO_CLIENT)])
        assert as_text(t) == o.text(), r
    # sizing call, a buffer too small, then the real call
    arr = np.array([(0, 0, 0, TEXT, 3, 500), (0, 0, 0, TEXT, 0, 2)], dtype=mte.VIEW_Q_DTYPE)
    out = np.zeros(2, dtype=mte.VIEW_R_DTYPE)
    n = ctypes.c_size_t()
    L = mte.lib()
    assert L.mte_views(engine._h, arr.ctypes.data, 2, out.ctypes.data, None, 0, ctypes.byref(n)) == 0
    v = views.View(rows, 0, OBSERVER)
    want = v.text(3, 500) + v.text(0, 2)
    assert n.value == len(want) > 400 and [int(x) for x in out["length"]] == [len(v.text(3, 500)), 2]
    buf = np.zeros(n.value, dtype=np.uint16)
    assert L.mte_views(engine._h, arr.ctypes.data, 2, out.ctypes.data, buf.ctypes.data, 100, ctypes.byref(n)) == -7
    assert n.value == len(want)
    assert L.mte_views(engine._h, arr.ctypes.data, 2, out.ctypes.data, buf.ctypes.data, len(want), ctypes.byref(n)) == 0
    assert buf.tolist() == want and [int(x) for x in out["text_off"]] == [0, len(want) - 2]
    check_no_download(engine, [rows, []])


def test_group_sizes_and_refusals(engine):
    log = views.no_msn(random_json_log(3, 400, n_writers=8, emoji=False))
    rows = table(log)
    small = [[msg("a", 1, 0, ins(0, "hello")), msg("b", 2, 1, ins(2, "XY")), msg("a", 3, 2, rem(0, 1))] for _ in range(300)]
    failing = [msg("w", 1, 0, ins(0, "ab")), msg("w", 2, 1, ins(5, "x"))]  # MergeTree insert failed
    logs = [log] + small + [[], failing, []]
    load(engine, logs)
    d_fail = len(logs) - 2
    assert engine.status(d_fail)[0] == 1
    tables = [rows] + [table(small[0])] * 300 + [[], None, []]
    rng = random.Random(5)
    L = views.length(rows, 400, "w3")
    for n in (1, 63, 64, 65, 1000):  # probes of ONE group, with duplicates, shuffled: out[i] answers q[i]
        pos = [rng.randint(0, L + 3) for _ in range(n)]
        pos = [rng.choice(pos) if i % 4 == 0 else p for i, p in enumerate(pos)]
        q = [(0, 400, "w3", LOCATE, p, 0) for p in pos]
        res, _ = views.check_views(engine, tables, q)
        assert len(res) == n
    # one query for each of 300 small documents, beside empty documents and a failed one
    q = [(d, 3, rng.choice(["a", "b", OBSERVER, None]), rng.choice([LENGTH, LOCATE, TEXT]), rng.randint(0, 6), 9)
         for d in range(1, 301)] + [(301, 0, OBSERVER, LENGTH, 0, 0), (303, 0, None, LOCATE, 0, 0)]
    rng.shuffle(q)
    views.check_views(engine, tables, q)
    bad = [(d_fail, 0, 0, LENGTH, 0, 0),                                   # -> DOC_FAILED
           (len(logs), 0, 0, LENGTH, 0, 0), (0, 0, 128, LENGTH, 0, 0),     # doc, client out of range
           (0, 0, 0, 3, 0, 0), (0, 0, 0, TEXT, 5, 4),                      # unknown kind, pos2 < pos1
           (0, 0, 0, LENGTH, 0, 0)]
    res, txt = engine.views(bad)
    assert [int(s) for s in res["status"]] == [views.DOC_FAILED] + [views.BAD_QUERY] * 4 + [views.OK]
    assert int(res["length"][5]) == views.length(rows, 0, OBSERVER) and len(txt) == 0
    assert engine.get_info("downloaded") == 0


def test_before_a_replay():
    e = mte.Engine(0)
    try:
        with pytest.raises(mte.MteError, match=r"\(-4\)"):  # MTE_E_STATE
            e.views([(0, 0, 0, LENGTH, 0, 0)])
        b = mte.Builder()
        b.add_doc([msg("a", 1, 0, ins(0, "x"))], observer=OBSERVER)
        e.load(b.batch())
        with pytest.raises(mte.MteError, match=r"\(-4\)"):
            e.views([(0, 0, 0, LENGTH, 0, 0)])
        with pytest.raises(mte.MteError, match=r"\(-4\)"):
            e.view_props(0, 0)
    finally:
        e.close()


def test_facade():
    """MergeTreeClient's positional reads on the SharedString spec's annotate case."""
    from tests.test_sharedstring_spec import CASES

    c = mte.MergeTreeClient(observer=OBSERVER)
    try:
        for m in CASES["annotate"][0]:
            c.applyMsg(m)
        for i in range(11):
            want = {"style": "bold", "color": "green"} if i >= 6 else {"style": "bold"}
            assert c.getPropertiesAtPosition(i) == want, i
        assert c.getPropertiesAtPosition(11) is None
        assert c.getText(6, 11) == "world" and c.getText() == "hello world" and c.getText(6) == "world"
        assert c.getContainingSegment(11) == (None, None)
        row, off = c.getContainingSegment(8)
        assert (row, off) == (1, 2) and c.getPosition(row) == 6
        assert c.getLengthAt(1, "s1") == 11 and c.getLengthAt(2, "s1") == 11
        c.applyMsg(msg("s2", 3, 2, ins(0, "oh, "), 1))
        assert c.getText(0, 9) == "oh, hello" and c.getLengthAt(2, "s1") == 11 and c.getLengthAt(2, "s2") == 15
        assert c.getPropertiesAtPosition(0) is None
    finally:
        c._engine.close()
