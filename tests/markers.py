"""The marker queries (mte_markers: findTile and getTextAndMarkers) restated in Python over a segment
table -- the rows of the oracle's segments_json() -- and the logs the marker tests share. All of it is the
observer's current view: a row's length is its local net length, 0 when it is removed at all.

find_tile walks the rows as the reference's search / backwardSearch walk the leaves of one block
(mergeTree.ts:1791-1874 with tileShift / recordTileStart, :996-1035); paragraphs is mapRange with gatherText
in parallelArrays mode (textSegment.ts:127-152, 188-275), its tag lists kept as the lists they are there."""
import json
import random

from tests.oplog import ann, ins, msg, rem
from tests.views import units

OBSERVER = "obs"
TILE_BEFORE, TILE_AFTER, PARAGRAPHS = 0, 1, 2
OK, NOT_FOUND, UNSUPPORTED, DOC_FAILED, BAD_QUERY = 0, 1, 2, 3, 4
F_REMOVED = 1
TO_END = 0xFFFFFFFF
TILE_KEY = "referenceTileLabels"


def props_of(row):
    return json.loads(row["props"]) if row.get("props") else None


def truthy(v):
    """JavaScript truthiness of a JSON value."""
    return not (v is None or v is False or v == 0 or v == "")


def net_len(row):
    return 0 if "removedSeq" in row else row["len"]


def has_tile_label(row, label):
    """refHasTileLabel (mergeTree.ts:581-597). `for (x of value)`: the elements of an array, the code points
    of a string; any other truthy value throws in the reference and matches nothing here."""
    if row["kind"] != "M" or not row["refType"] & 1:
        return False
    p = props_of(row)
    v = p.get(TILE_KEY) if p else None
    if not truthy(v):
        return False
    if isinstance(v, list):
        return any(isinstance(x, str) and x == label for x in v)
    if isinstance(v, str):
        return any(c == label for c in v)
    return False


def find_tile(rows, pos, label, preceding=True):
    """(row, position of the row) or None."""
    tile = None
    if preceding:
        p = pos
        for i, r in enumerate(rows):
            n = net_len(r)
            if p < n:  # the containing leaf: recordTileStart
                if has_tile_label(r, label):
                    tile = i
                break
            if n > 0 and has_tile_label(r, label):  # tileShift of a passed leaf
                tile = i
            p -= n
    else:
        end = sum(net_len(r) for r in rows)
        if pos > end:
            return None
        for i in range(len(rows) - 1, -1, -1):
            n = net_len(rows[i])
            start = end - n
            if pos >= start:  # the containing leaf, whatever its length: recordTileStart tests no visibility
                if has_tile_label(rows[i], label):
                    tile = i
                break
            if n > 0 and has_tile_label(rows[i], label):
                tile = i
            end = start
    if tile is None:
        return None
    return tile, sum(net_len(r) for r in rows[:tile])


def gather_tags(props, in_progress):
    """gatherText's tag block (textSegment.ts:196-240), verbatim on lists: returns endTags + beginTags and
    updates in_progress."""
    tags, init, rem_tags = [], [], []
    begin = end = ""
    if props and truthy(props.get("font-weight")):
        tags.append("b")
    if props and truthy(props.get("text-decoration")):
        tags.append("u")
    if tags:
        for t in tags:
            if t not in in_progress:
                begin += f"<{t}>"
                init.append(t)
        for t in in_progress:
            if t not in tags:
                end += f"</{t}>"
                rem_tags.append(t)
        for t in reversed(init):
            in_progress.append(t)
    else:
        for t in in_progress:
            end += f"</{t}>"
            rem_tags.append(t)
    for t in rem_tags:
        if t in in_progress:
            in_progress.remove(t)
    return end + begin


def paragraphs(rows, label, start=0, end=TO_END):
    """getTextAndMarkers(label, start, end): [dict(row, pos, units)], one per visible tile of [start, end);
    the text behind the last tile is dropped."""
    out, text, in_progress, at = [], [], [], 0
    for i, r in enumerate(rows):
        n = net_len(r)
        lo, hi = max(at, start), min(at + n, end)
        if lo < hi:  # mapRange visits the rows that overlap the range
            if r["kind"] == "T":
                text += units(gather_tags(props_of(r), in_progress)) + units(r["text"])[lo - at: hi - at]
            elif r["kind"] == "M" and has_tile_label(r, label):
                out.append(dict(row=i, pos=at, units=text))
                text = []
        at += n
    return out


def expect(rows, kind, pos1, pos2, label):
    """What mte_markers answers on a replayed, unrefused document."""
    if kind == PARAGRAPHS:
        return dict(status=OK, pieces=paragraphs(rows, label, pos1, pos2))
    t = find_tile(rows, pos1, label, kind == TILE_BEFORE)
    if t is None:
        return dict(status=NOT_FOUND, row=0, pos=0, flags=0)
    return dict(status=OK, row=t[0], pos=t[1], flags=F_REMOVED if "removedSeq" in rows[t[0]] else 0)


def check_markers(engine, tables, queries, labels):
    """One mte_markers call for all `queries` -- (doc, kind, pos1, pos2, label index) -- against expect() on
    tables[doc] (the oracle's rows of the same log). No query may come back UNSUPPORTED: the builders here
    never annotate the tile-label key. Returns the results."""
    res, pieces, text = engine.markers(queries, labels)
    assert len(res) == len(queries)
    assert sum(int(s) == UNSUPPORTED for s in res["status"]) == 0  # the refusal cap of these tests: none
    n_p = n_t = 0
    for i, (d, kind, p1, p2, li) in enumerate(queries):
        want = expect(tables[d], kind, p1, p2, labels[li])
        got = res[i]
        assert int(got["status"]) == want["status"], (i, queries[i], {x: int(got[x]) for x in got.dtype.names}, want)
        if kind != PARAGRAPHS:
            for f in ("row", "pos", "flags"):
                assert int(got[f]) == want[f], (i, queries[i], f, {x: int(got[x]) for x in got.dtype.names}, want)
            continue
        assert int(got["count"]) == len(want["pieces"]), (i, queries[i], int(got["count"]), len(want["pieces"]))
        assert int(got["first_piece"]) == n_p, (i, queries[i])
        for w in want["pieces"]:
            p = pieces[n_p]
            assert (int(p["row"]), int(p["pos"])) == (w["row"], w["pos"]), (i, queries[i], n_p)
            assert int(p["text_off"]) == n_t and int(p["text_len"]) == len(w["units"]), (i, queries[i], n_p)
            assert text[n_t: n_t + len(w["units"])].tolist() == w["units"], (i, queries[i], n_p)
            n_p += 1
            n_t += len(w["units"])
    assert n_p == len(pieces) and n_t == len(text)
    return res, pieces, text


# ---- logs

def tile(labels=("EOP",), ref_type=1, **more):
    """A marker segment: ReferenceType.Tile with referenceTileLabels = labels (a list, or any JSON value)."""
    return {"marker": {"refType": ref_type}, "props": dict({TILE_KEY: list(labels) if isinstance(labels, tuple) else labels}, **more)}


def text_seg(s, bold=None, under=None):
    p = {}
    if bold is not None:
        p["font-weight"] = bold
    if under is not None:
        p["text-decoration"] = under
    return {"text": s, "props": p} if p else s


class Writer:
    """One writer whose every op sees all before it (refSeq = seq - 1), MSN 0 unless told: rows never
    merge, so the row a segment lands on is its insertion order's."""

    def __init__(self, name="w"):
        self.name, self.seq, self.log, self.length = name, 0, [], 0

    def _put(self, contents, msn=0, client=None):
        self.seq += 1
        self.log.append(msg(client or self.name, self.seq, self.seq - 1, contents, msn))

    def insert(self, pos, seg, msn=0):
        self._put(ins(pos, seg), msn)
        self.length += 1 if isinstance(seg, dict) and "marker" in seg else len(units(seg["text"] if isinstance(seg, dict) else seg))

    def append(self, seg, msn=0):
        self.insert(self.length, seg, msn)

    def remove(self, a, b, client=None):
        self._put(rem(a, b), client=client)
        self.length -= b - a

    def annotate(self, a, b, props):
        self._put(ann(a, b, props))


def seam_log(n=140, tiles=(0, 62, 63, 64, 65)):
    """n rows (MSN 0: none merges): a tile on each row of `tiles` and on the last row, two-unit text rows
    elsewhere, so tiles sit on both sides of the 64-row step and probes land on every side of them."""
    w = Writer()
    for i in range(n):
        if i in tiles or i == n - 1:
            w.append(tile())
        else:
            w.append(chr(97 + i % 26) + chr(65 + i % 26))
    return w.log


def tiled(log, seed, labels=("EOP", "H1", "\U0001F600")):
    """A random JSON log (tests/test_gpu_fuzz.random_json_log) with tiles and tags added, no position or
    length changed: a share of its markers and of its one-unit text inserts becomes Tile markers carrying referenceTileLabels (arrays,
    strings, other values), and its annotates' "bold" / "size" keys become the two tag properties."""
    rng = random.Random(seed)
    values = [[labels[0]], [labels[0]], [labels[1], labels[0]], list(labels), [labels[1]], labels[0][0], labels[2] + "x", "", None, 7, True,
              {"a": 1}, []]

    def fix(op):
        if op.get("type") == 3:
            return dict(op, ops=[fix(o) for o in op["ops"]])
        seg = op.get("seg")
        one_unit = isinstance(seg, dict) and "text" in seg and len(units(seg["text"])) == 1  # as long as a marker
        if isinstance(seg, dict) and (("marker" in seg and rng.random() < 0.8) or (one_unit and rng.random() < 0.5)):
            seg = {"marker": {"refType": rng.choice([1, 1, 1, 3, 0, 2])}, "props": {"x": 1, TILE_KEY: rng.choice(values)}}
            return dict(op, seg=seg)
        if op.get("type") == 2:
            names = {"bold": "font-weight", "size": "text-decoration"}
            return dict(op, props={names.get(k, k): v for k, v in op["props"].items()})
        return op

    return [dict(m, contents=fix(m["contents"])) for m in log]
