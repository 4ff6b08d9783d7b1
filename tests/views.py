"""The view queries (mte_views: length, position and text as any client saw them) restated in Python
over a segment table -- the rows of the oracle's segments_json(), which name clients by long id -- and
the logs the view tests share. A view is (ref_seq, client): client OBSERVER is the local view (ref_seq
unused), None a client that owns no slot of the document (MTE_VIEW_NO_CLIENT), else a writer's long id.
The view length of a row is the reference's nodeLength (mergeTree.ts:1659-1699)."""
import bisect
import json

from tests.oplog import ins, msg, rem

OBSERVER = "obs"
LENGTH, LOCATE, TEXT = 0, 1, 2
OK, PAST_END, OUT_OF_WINDOW, DOC_FAILED, BAD_QUERY = 0, 1, 2, 3, 4
NO_CLIENT = 0xFFFFFFFF
F_REMOVED = 1


def rows_of(oracle_doc):
    return json.loads(oracle_doc.segments_json())


def units(s):
    """A Python string as UTF-16 code units."""
    b = s.encode("utf-16-le", "surrogatepass")
    return [b[i] | b[i + 1] << 8 for i in range(0, len(b), 2)]


def view_len(row, ref_seq, client, observer=OBSERVER):
    removed = "removedSeq" in row
    if client == observer or row["client"] == "original":  # the local view
        return 0 if removed else row["len"]
    if not (row["client"] == client or row["seq"] <= ref_seq):
        return 0
    if removed and (row["removedClient"] == client or client in row["overlap"] or row["removedSeq"] <= ref_seq):
        return 0
    return row["len"]


class View:
    """One view of a segment table, prepared once: every row's view length, the cumulative ends, the
    observer-visible units before each row, and the view's units (None where a marker or run counts)."""

    def __init__(self, rows, ref_seq, client, observer=OBSERVER):
        self.rows = rows
        self.ends, self.cur, self.unit_at = [], [], []
        at = cur = 0
        for r in rows:
            v = view_len(r, ref_seq, client, observer)
            at += v
            self.ends.append(at)
            self.cur.append(cur)
            cur += 0 if "removedSeq" in r else r["len"]
            if v:
                self.unit_at += units(r["text"]) if r["kind"] == "T" else [None] * v
        self.length = at
        assert len(self.unit_at) == at

    def locate(self, pos):
        """getContainingSegment + getPosition: dict(status, row, offset, length, cur_pos, flags). The first
        row whose cumulative end exceeds pos: rows of length 0 in the view are skipped."""
        if pos >= self.length:
            return dict(status=PAST_END, row=0, offset=0, length=self.length, cur_pos=0, flags=0)
        i = bisect.bisect_right(self.ends, pos)
        r = self.rows[i]
        return dict(status=OK, row=i, offset=pos - (self.ends[i] - r["len"]), length=r["len"], cur_pos=self.cur[i],
                    flags=F_REMOVED if "removedSeq" in r else 0)

    def text(self, pos1=0, pos2=NO_CLIENT):
        """MergeTreeTextHelper.getText(ref_seq, client, "", pos1, pos2) as UTF-16 units."""
        return [u for u in self.unit_at[pos1:pos2] if u is not None]

    def expect(self, kind, pos1, pos2):
        """What mte_views answers on a replayed, in-window document: dict(status, row, offset, length,
        cur_pos, flags) and, for TEXT, units."""
        if kind == LENGTH:
            return dict(status=OK, row=0, offset=0, length=self.length, cur_pos=0, flags=0)
        if kind == LOCATE:
            return self.locate(pos1)
        u = self.text(pos1, pos2)
        return dict(status=OK, row=0, offset=0, length=len(u), cur_pos=0, flags=0, units=u)


def length(rows, ref_seq, client, observer=OBSERVER):
    return View(rows, ref_seq, client, observer).length


def text(rows, ref_seq, client, pos1=0, pos2=NO_CLIENT, observer=OBSERVER):
    return View(rows, ref_seq, client, observer).text(pos1, pos2)


def check_views(engine, tables, queries):
    """One mte_views call for all `queries` -- (doc, ref_seq, client long id / OBSERVER / None, kind, pos1,
    pos2) -- against expect() on tables[doc] (the oracle's rows of the same log). Returns the results."""
    slots = {}

    def slot(d, c):
        if c is None:
            return NO_CLIENT
        if (d, c) not in slots:
            slots[d, c] = 0 if c == OBSERVER else engine.client_slot(d, c)
        return slots[d, c]

    res, txt = engine.views([(d, r, slot(d, c), k, p1, p2) for d, r, c, k, p1, p2 in queries])
    assert len(res) == len(queries)
    laid, prepared = 0, {}
    for i, (d, r, c, k, p1, p2) in enumerate(queries):
        if (d, r, c) not in prepared:
            prepared[d, r, c] = View(tables[d], r, c)
        want = prepared[d, r, c].expect(k, p1, p2)
        got = res[i]
        for f in ("status", "row", "offset", "length", "cur_pos", "flags"):
            assert int(got[f]) == want[f], (i, queries[i], f, {x: int(got[x]) for x in got.dtype.names}, want)
        if k == TEXT:
            assert int(got["text_off"]) == laid, (i, queries[i])
            assert txt[laid: laid + want["length"]].tolist() == want["units"], (i, queries[i])
            laid += want["length"]
    assert laid == len(txt)
    return res, txt


def no_msn(log):
    """The log with every message's minimumSequenceNumber 0: nothing is ever merged or dropped."""
    return [dict(m, minimumSequenceNumber=0) for m in log]


SEAM_SIZES = (0, 1, 63, 64, 65, 128, 129, 200)
SEAM_WRITERS = ["w0", "w1"]
SEAM_REMOVERS = {62: "r0", 63: "r1", 64: "r2", 65: "r3", 126: "r4", 127: "r5", 128: "r6", 129: "r7"}


def seam_log(n):
    """n final rows: alternating writers append one two-unit insert each, MSN 0 throughout, so nothing
    merges; then rows 62..65 and 126..129 (those the document has) are removed, each by another client, so
    rows of length 0 in some views sit on both sides of every 64-row step."""
    out = []
    for i in range(n):
        out.append(msg(SEAM_WRITERS[i % 2], i + 1, i, ins(2 * i, chr(97 + i % 26) + chr(65 + i % 26)), 0))
    seq = n
    for row in sorted((r for r in SEAM_REMOVERS if r < n), reverse=True):  # (from the back: positions hold)
        seq += 1
        out.append(msg(SEAM_REMOVERS[row], seq, seq - 1, rem(2 * row, 2 * row + 2), 0))
    return out


def seam_views(log):
    """The seam tests' views: the observer; each client and no client at ref_seq 0, mid and cur_seq."""
    cur = len(log)
    names = sorted({m["clientId"] for m in log})
    return [(0, OBSERVER)] + [(r, c) for c in names + [None] for r in sorted({0, cur // 2, cur})]


def seam_queries(d, rows, log):
    """LENGTH and LOCATE at every position 0..L (L is past the end) in every seam view of document d."""
    q = []
    for r, c in seam_views(log):
        L = length(rows, r, c)
        q.append((d, r, c, LENGTH, 0, 0))
        q += [(d, r, c, LOCATE, p, 0) for p in range(L + 1)]
    return q
