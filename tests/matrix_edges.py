"""Log builders for tests/test_gpu_matrix_edges.py: SharedMatrix documents at the sizes where the cell
path changes course -- block lists past 64 and 128 leaf blocks, handles past each
SparseArray2D level, engineered handle recycling, writers in every band of the removers words --
each with a closed-form expectation beside the oracle's, and the numbers (`facts`) that
tests/test_matrix_edges_cpu.py pins so that a builder cannot silently fall below its seam.

The closed forms come from Model, a positional restatement that knows nothing of segments, blocks
or zamboni: a row is an id with the seq / client of its insert and of every remove that hit it, a
view is a filter over those, a `set` lands where both positions are defined (matrix.ts:575-601) and
the first defined set of a row takes the next handle of its vector's table (handletable.ts:35-59).
It is valid for logs whose inserts are sequenced with refSeq = seq - 1 (no concurrent inserts: no
tie-break), which every builder here keeps to."""
import json
import random

from oracle import OracleMatrix
from tests.oplog import dumps, msg
from tests.test_matrix import UNALLOC, splice_ins, splice_rem  # noqa: F401 (UNALLOC: for the tests)
from tests.test_matrix_spec import grid, vector_handles

LEAF_SLOTS = 8  # segments per leaf block


class _Item:
    __slots__ = ("id", "seq", "client", "rem", "handle")

    def __init__(self, id_, seq, client):
        self.id, self.seq, self.client, self.rem, self.handle = id_, seq, client, {}, None


class Model:
    """Both vectors as lists of _Item in document order, the cells by (row id, col id)."""

    def __init__(self):
        self.ax = {"rows": [], "cols": []}
        self.free = {"rows": [], "cols": []}   # freed handles, last freed last (the table is LIFO)
        self.top = {"rows": 1, "cols": 1}      # next never-used handle
        self.cells = {}
        self.n_id = 0
        self.undefined = 0                     # sets that found a position undefined
        self.allocs = {"rows": [], "cols": []}  # handles in allocation order

    @staticmethod
    def _sees(it, ref, client):
        if it.seq > ref and it.client != client:
            return False
        return not any(s <= ref or c == client for c, s in it.rem.items())

    def view(self, axis, ref, client):
        return [it for it in self.ax[axis] if self._sees(it, ref, client)]

    def insert(self, axis, pos, n, seq, client):
        v = self.view(axis, seq - 1, client)
        at = self.ax[axis].index(v[pos - 1]) + 1 if pos else 0  # before any tombstone at pos
        new = [_Item(self.n_id + i, seq, client) for i in range(n)]
        self.n_id += n
        self.ax[axis][at:at] = new

    def remove(self, axis, a, b, seq, client, ref):
        for it in self.view(axis, ref, client)[a:b]:
            it.rem.setdefault(client, seq)

    def _alloc(self, axis, it):
        if it.handle is None:
            it.handle = self.free[axis].pop() if self.free[axis] else self.top[axis]
            if it.handle == self.top[axis]:
                self.top[axis] += 1
            self.allocs[axis].append(it.handle)

    def set(self, r, c, value, client, ref):
        row = self.view("rows", ref, client)[r]
        if row.rem:                      # removed concurrently: adjustPosition undefined, cols not looked at
            self.undefined += 1
            return False
        col = self.view("cols", ref, client)[c]
        if col.rem:
            self.undefined += 1
            return False
        self._alloc("rows", row)
        self._alloc("cols", col)
        self.cells[(row.id, col.id)] = value
        return True

    def unlink(self, axis, items):
        """Zamboni's UNLINK of removed rows, in document order: their handles go back, their cells go."""
        for it in items:
            assert it.rem
            if it.handle is not None:
                self.free[axis].append(it.handle)
                self.cells = {k: v for k, v in self.cells.items() if k[axis == "cols"] != it.id}
            self.ax[axis].remove(it)

    def table(self, axis):
        """HandleTable.snapshot(): [head of the free list, then per handle 0 (in use) or its link]."""
        t = [0] * self.top[axis]
        nxt = self.top[axis]
        for h in self.free[axis]:
            t[h] = nxt
            nxt = h
        t[0] = nxt
        return t

    def live(self, axis):
        return [it for it in self.ax[axis] if not it.rem]

    def grid(self):
        return [[self.cells.get((r.id, c.id)) for c in self.live("cols")] for r in self.live("rows")]

    def handles(self, axis):
        return [it.handle for it in self.live(axis)]


class Log:
    """Messages and the Model side by side. ref None: the writer has seen everything (seq - 1)."""

    def __init__(self):
        self.msgs, self.seq, self.msn, self.m = [], 0, 0, Model()
        self.follow = True   # the MSN follows the sequence number (one settled writer)

    def _push(self, w, contents, ref):
        self.seq += 1
        ref = self.seq - 1 if ref is None else ref
        if self.follow:
            self.msn = self.seq - 1
        self.msgs.append(msg(w, self.seq, ref, contents, self.msn))
        return ref

    def insert(self, w, axis, pos, n):
        self._push(w, splice_ins(axis, pos, n), None)
        self.m.insert(axis, pos, n, self.seq, w)

    def remove(self, w, axis, a, b, ref=None):
        ref = self._push(w, splice_rem(axis, a, b), ref)
        self.m.remove(axis, a, b, self.seq, w, ref)

    def set(self, w, r, c, value, ref=None):
        ref = self._push(w, {"type": 2, "row": r, "col": c, "value": value}, ref)
        return self.m.set(r, c, value, w, ref)

    def tail(self, w, n=1):
        """Empty removes that carry the MSN up to the sequence number: zamboni unlinks what it reaches."""
        self.follow = True
        for _ in range(n):
            self._push(w, splice_rem("rows", 0, 0), None)


class Doc:
    """A built document: log, closed-form grid / visible handles / handle tables (None where the
    builder states none) and `facts`, the numbers that make it an edge."""

    def __init__(self, name, log, want_grid=None, want_handles=None, want_tables=None, facts=None):
        self.name, self.log = name, log
        self.want_grid, self.want_handles, self.want_tables = want_grid, want_handles, want_tables
        self.facts = facts or {}
        self.want_cells = None   # {(row handle, col handle): value}: every cell of the blob that is not null


def oracle(log, observer="obs"):
    o = OracleMatrix(observer)
    assert o.apply_json(dumps(log)) == 0, (o.rows.status(), o.cols.status())
    return o


def tables(summary):
    """{"rows": [...], "cols": [...]}: the handleTable blobs of a matrix summary tree."""
    ents = {e["path"]: e["value"] for e in summary["entries"]}
    return {a: json.loads(ents[a]["entries"][1]["value"]["contents"]) for a in ("rows", "cols")}


def handles(summary):
    ents = {e["path"]: e["value"] for e in summary["entries"]}
    return {a: vector_handles(ents[a]) for a in ("rows", "cols")}


def blob_cells(summary):
    """{(row handle, col handle): value} of every non-null cell of the cells blob (the inverse of
    r0c0ToMorton2x16, sparsearray2d.ts:20-36, over the five levels)."""
    ents = {e["path"]: e["value"] for e in summary["entries"]}
    root = json.loads(ents["cells"]["contents"])[0]

    def split(key):  # odd bits: row, even bits: col
        r = c = 0
        for i in range(16):
            c |= ((key >> (2 * i)) & 1) << i
            r |= ((key >> (2 * i + 1)) & 1) << i
        return r, c

    out = {}
    for i0, l0 in enumerate(root):
        for i1, l1 in enumerate(l0 or []):
            for i2, l2 in enumerate(l1 or []):
                for i3, l3 in enumerate(l2 or []):
                    for i4, v in enumerate(l3 or []):
                        if v is not None:
                            rh, ch = split(i0)
                            r, c = split(i1 << 24 | i2 << 16 | i3 << 8 | i4)
                            out[(rh << 16 | r, ch << 16 | c)] = v
    return out


def n_segments(vec):
    return len(json.loads(vec.segments_json()))


# ------------------------------------------------------------------------------- fragmented vector
def fragmented(n, seed=1):
    """One run of n rows and 3 cols; sets at the even rows in a shuffled order (handles never
    contiguous: every row ends a segment of its own). Half way: a settled writer and a concurrent one
    remove rows near the front, then sets from lagging views land beyond the removed rows (adjusted
    position != raw), into them (undefined), and from the settled view. Removed rows are unlinked by
    the tail only, so the i-th allocation takes handle i."""
    rng = random.Random(seed)
    g = Log()
    g.insert("w0", "rows", 0, n)
    g.insert("w0", "cols", 0, 3)
    even = list(range(0, n, 2))
    rng.shuffle(even)
    half = len(even) // 2
    for i, r in enumerate(even[:half]):
        g.set("w0", r, i % 3, i)
    # the removes: w0 settled, w1 concurrent with it (both against the same refSeq); the MSN stays
    g.follow = False
    ref0 = g.seq
    g.remove("w0", "rows", 8, 14, ref=ref0)
    g.remove("w1", "rows", 11, 20, ref=ref0)     # overlaps w0's
    g.remove("w1", "rows", 31, 35, ref=ref0)     # rows 40..43: its view already lacks its own 11..19
    rest = [r for r in even[half:] if r >= 48]
    und0 = g.m.undefined
    moved = 0
    for i, r in enumerate(rest):
        k = i % 3
        if k == 0:      # w2 has seen none of the removes: raw position, adjusted by 16 rows
            g.set("w2", r, i % 3, f"a{i}", ref=ref0)
            moved += 1
        elif k == 1:    # w1 has seen only its own: its view lacks rows 11..19 and 40..43
            g.set("w1", r - 13, (i + 1) % 3, f"b{i}", ref=ref0)
            moved += 1
        else:           # w0 has seen everything
            g.set("w0", r - 16, (i + 2) % 3, f"c{i}", ref=None)
    # lagging sets INTO removed rows: undefined, no handle. w2 sees rows 9 (w0's), 15 and 41 (w1's);
    # w1 still sees row 8 (w0's alone); w0's view lacks its own 8..13, so its position 8 is row 14,
    # which w1 removed. The last one is defined: w0's position 15 is row 21, an odd row (a new handle).
    for w, r in (("w2", 9), ("w2", 15), ("w2", 41), ("w1", 8), ("w0", 8), ("w0", 15)):
        g.set(w, r, 0, f"late{r}", ref=ref0)
    und = g.m.undefined - und0
    g.tail("w0", 4)
    m = g.m
    o = oracle(g.msgs)
    return Doc(f"frag{n}", g.msgs, m.grid(), {"rows": m.handles("rows"), "cols": m.handles("cols")}, None,
               {"row_segments": n_segments(o.rows), "undefined": und, "moved": moved,
                "row_allocs": len(m.allocs["rows"]), "msgs": len(g.msgs)})


# ---------------------------------------------------------------------------- long before any set
def spliced(n=700, back=90, seed=None):
    """A row vector that is long from its splices alone, which is all pass 1 (adjustPosition) sees:
    n single-row inserts with the MSN held at 0 -- at the end, or with a seed at random positions,
    which fills the leaf blocks better -- so zamboni merges none of them and the vector is n
    segments, more than 64 leaf blocks of 8, before the first set. Then overlapping
    removes near the end by a settled and a concurrent writer, and sets at positions past segment
    8 x 64 from views before the removes (adjusted != raw: the prefix sums every block in front, the
    second 64 included), from the removers' views, into the removed rows (undefined), and from the
    current view; a few sets near the front for contrast. The tail carries the MSN up."""
    rng = random.Random(seed)
    g = Log()
    g.follow = False
    g.insert("w0", "cols", 0, 3)
    for i in range(n):
        g.insert("w0", "rows", i if seed is None else rng.randint(0, i), 1)
    first_set = len(g.msgs)
    ref0 = g.seq
    a = n - back                                   # the hole: rows a .. a + 19, far past segment 512
    g.remove("w0", "rows", a, a + 12, ref=ref0)
    g.remove("w1", "rows", a + 8, a + 20, ref=ref0)
    und0, moved, far = g.m.undefined, 0, []
    for i, r in enumerate(range(a + 22, n, 5)):    # beyond the hole
        w = ("w2", "w1", "w0")[i % 3]              # w2 sees no remove, w1 and w0 only their own 12
        pos = r if w == "w2" else r - 12
        moved += g.set(w, pos, i % 3, f"far{i}", ref=ref0)
        far.append(pos)
    for i, r in enumerate(range(a + 21, n, 7)):    # the current view: all 20 rows gone
        if (r - a - 22) % 5 == 0:                  # (a row the lagging sets wrote: keep their values)
            continue
        g.set("w0", r - 20, (i + 1) % 3, f"now{i}")
        far.append(r - 20)
    for w, r in (("w2", a + 3), ("w2", a + 15), ("w1", a + 2), ("w0", a + 2)):
        g.set(w, r, 0, f"gone{r}", ref=ref0)       # into the hole (w0's position a + 2 is row a + 14: w1's)
    und = g.m.undefined - und0
    for r in (0, 5, 63):
        g.set("w2", r, 1, f"near{r}", ref=ref0)
    g.tail("w0", 4)
    m = g.m
    name = f"spliced{n}" + ("" if seed is None else "r")
    return Doc(name, g.msgs, m.grid(), {"rows": m.handles("rows"), "cols": m.handles("cols")}, None,
               {"first_set": first_set, "undefined": und, "moved": moved, "min_far": min(far)})


# ----------------------------------------------------------------------------------- handle levels
LEVELS = (16, 256, 4096)


def handle_levels(n=4200):
    """n rows x n cols, set along the diagonal in order: row i and col i take handle i + 1 and both
    tables pass 16, 256 and 4 096. Then the four cells around each boundary on both axes, and cells
    whose handle is past a boundary on one axis only. The closed form is by handle (`want_cells`:
    (row handle, col handle) -> value; a 4 200 x 4 200 grid is 17 M reads), stated without the Model."""
    g = Log()
    g._push("w0", splice_ins("rows", 0, n), None)
    g._push("w0", splice_ins("cols", 0, n), None)
    cells = {}

    def put(hr, hc, v):     # handle h sits at position h - 1
        g._push("w0", {"type": 2, "row": hr - 1, "col": hc - 1, "value": v}, None)
        cells[(hr, hc)] = v

    for h in range(1, n + 1):
        put(h, h, h)
    corner = []
    for b in LEVELS:
        corner += [(hr, hc) for hr in (b - 1, b) for hc in (b - 1, b) if hr != hc]
        corner += [(b + 3, 2), (2, b + 3), (b + 3, b // 4 + 1), (b // 4 + 1, b + 3)]
    for hr, hc in corner:
        put(hr, hc, f"{hr}/{hc}")
    g.tail("w0", 2)
    hs = list(range(1, n + 1))
    d = Doc(f"levels{n}", g.msgs, None, {"rows": hs, "cols": hs}, {"rows": [n + 1] + [0] * n, "cols": [n + 1] + [0] * n},
            {"corner": corner, "row_table": n + 1, "col_table": n + 1})
    d.want_cells = cells
    return d


def big_handle_summary(n=65600):
    """(summary, suffix, expectation): an oracle-made summary of a tiny matrix whose rows vector is
    rewritten to one run [n, 1] with a handle table of that length (every handle in use), so the
    suffix's sets meet row handles >= 65 536 (root index > 0, the key's high half) without a
    65 600-set log. The suffix sets cells either side of 65 536, removes a sub-range that straddles
    it (handles 65 534 .. 65 538) and lets zamboni unlink it."""
    g = Log()
    g.insert("w0", "rows", 0, 4)
    g.insert("w0", "cols", 0, 3)
    for i in range(4):
        g.set("w0", i, 0, i)
    g.tail("w0", 3)
    base = json.loads(oracle(g.msgs).snapshot_json())
    ents = {e["path"]: e["value"] for e in base["entries"]}
    hdr = ents["rows"]["entries"][0]["value"]["entries"][0]["value"]
    h = json.loads(hdr["contents"])
    assert h["segments"] == [[4, 1]], h["segments"]
    h["segments"] = [[n, 1]]
    h["length"] = h["headerMetadata"]["totalLength"] = n
    hdr["contents"] = json.dumps(h, separators=(",", ":"))
    ents["rows"]["entries"][1]["value"]["contents"] = json.dumps([n + 1] + [0] * n, separators=(",", ":"))
    summary = json.dumps(base, separators=(",", ":"))
    seq0 = g.seq
    s = Log()
    s.seq = s.msn = seq0
    # position p holds handle p + 1. The removed positions 65533 .. 65537 hold handles 65534 .. 65538:
    # the range straddles 65 536, so its UNLINK clears a cell under root index 0 and one under index 2
    sets = [(65531, 0, "lo"), (65534, 1, "cutlo"), (65535, 2, "cuthi"), (65539, 1, "hi0"), (65540, 2, "hi1"),
            (n - 1, 0, "end")]
    for r, c, v in sets:
        s._push("w0", {"type": 2, "row": r, "col": c, "value": v}, None)
    s._push("w0", splice_rem("rows", 65533, 65538), None)
    s.tail("w0", 4)
    s._push("w0", {"type": 2, "row": 0, "col": 2, "value": "after"}, None)
    freed = list(range(65534, 65539))
    table = [n + 1] + [0] * n
    nxt = n + 1
    for hd in freed:
        table[hd] = nxt
        nxt = hd
    table[0] = nxt
    # by (row handle, col handle): col 0 took handle 1 in the base matrix, cols 1 and 2 take 2 and 3
    # here, in the order the sets meet them
    want = {(i + 1, 1): i for i in range(4)}
    want.update({(r + 1, c + 1): v for r, c, v in sets if not v.startswith("cut")})
    want[(1, 3)] = "after"
    return summary, s.msgs, {"rows_table": table, "cols_table": [4, 0, 0, 0], "cells": want, "rows": n - 5}


# --------------------------------------------------------------------------------------- recycling
def recycling(n=24):
    """Coalesced multi-handle runs over handles 1 .. n (sets in position order under a following MSN;
    zamboni merges inside a leaf block, so a run [length, start] holds 3 to 5 handles, never all n),
    removed below the MSN so the UNLINKs free 1 .. n in ascending order, then n + 1 allocations: the
    free list is LIFO, so they take n, n - 1, .., 1 and then n + 1. `cut` is the message index just
    after the UNLINKs: the prefix's table shows the whole free list, [n, n + 1, 1, 2, .., n - 1]."""
    g = Log()
    g.insert("w0", "rows", 0, n + 3)
    g.insert("w0", "cols", 0, 2)
    for i in range(n):
        g.set("w0", 1 + i, 0, f"old{i}")
    g.tail("w0", 3)                      # the runs settle and coalesce
    run_at = len(g.msgs)
    g.follow = False
    ref0 = g.seq
    g.remove("w0", "rows", 1, 1 + n, ref=ref0)
    ok = g.set("w1", 3, 1, "late", ref=ref0)     # w1 has not seen the remove: row 3 is gone, no handle
    assert not ok
    gone = [it for it in g.m.ax["rows"] if it.rem]
    g.tail("w0", 4)                      # the remove falls below the MSN: UNLINK
    g.m.unlink("rows", gone)
    cut = len(g.msgs)
    freed_table = g.m.table("rows")
    g.insert("w0", "rows", 1, n + 1)
    for i in range(n + 1):
        # even rows set the old key again (col 0: the col's handle 1), odd rows only col 1: their
        # (handle, col 0) cell stays cleared
        g.set("w0", 1 + i, i % 2, f"new{i}")
    g.tail("w0", 2)
    m = g.m
    return Doc(f"recycle{n}", g.msgs, m.grid(), {"rows": m.handles("rows"), "cols": m.handles("cols")},
               {"rows": m.table("rows"), "cols": m.table("cols")},
               {"n": n, "cut": cut, "run_at": run_at, "freed_table": freed_table,
                "realloc": m.allocs["rows"][n:], "undefined": m.undefined})


# ------------------------------------------------------------------------------------ many writers
def many_writers(nw=70, rows=60, cols=4):
    """nw writers, the MSN at 0 until all have written (every writer keeps its short id: slots up to
    nw). Writers of each band of the removers words (slots < 32, 32..63, >= 64 where nw allows) remove
    overlapping ranges against one refSeq; then writers of each band set cells from a view before the
    removes (into removed rows: undefined; beyond them: adjusted; the removers themselves: their own
    range is gone from their view, the others' is not) and from a view after them."""
    names = [f"w{i:02d}" for i in range(nw)]
    g = Log()
    g.follow = False
    g.insert(names[0], "rows", 0, rows)
    g.insert(names[0], "cols", 0, cols)
    for k, w in enumerate(names):                  # every writer writes: slot k + 1 in both vectors
        g.set(w, (7 * k) % rows, k % cols, k, ref=None)
    bands = [5, 40, 68] if nw >= 70 else [5, nw - 7, nw - 2]   # (40 writers: slots 6, 34 and 39)
    ref0 = g.seq
    for j, b in enumerate(bands):                  # rows 10..21, 14..25, 18..29: every pair overlaps
        g.remove(names[b], "rows", 10 + 4 * j, 22 + 4 * j, ref=ref0)
    g.remove(names[bands[-1]], "cols", 1, 2, ref=ref0)
    und0 = g.m.undefined
    n_def = 0
    for j, b in enumerate(bands):
        other, own = names[b + 1], names[b]
        for r in (12, 19, 28):                     # a bystander of the band, old view: removed rows
            n_def += g.set(other, r, 0, f"x{b}.{r}", ref=ref0)
        for r in (3, 33, rows - 1):                # ... and surviving rows before / after the hole
            n_def += g.set(other, r, 2, f"s{b}.{r}", ref=ref0)
        # the remover's old view lacks its own 12 rows: position 10 + 4j is the row after its range,
        # which another band removed unless this is the last band
        for r in (10 + 4 * j, 9, 30):
            n_def += g.set(own, r, 2, f"o{b}.{r}", ref=ref0)
        n_def += g.set(other, 1, 1, f"c{b}", ref=ref0)   # the removed col
        for r in (9, 10, 20):                      # after the removes: the current view
            n_def += g.set(other, r, 0, f"n{b}.{r}", ref=None)
    und = g.m.undefined - und0
    g.tail(names[0], 4)
    m = g.m
    return Doc(f"writers{nw}", g.msgs, m.grid(), None, None,
               {"names": names, "bands": [names[b] for b in bands], "undefined": und, "defined": n_def})


# ------------------------------------------------------------------------------------------ resume
def cuts():
    """(name, log, cut, the oracle's summary of log[:cut]) for the fragmented and the recycling
    document, cut in the middle."""
    out = []
    f = fragmented(FRAG_SIZES[-1])
    out.append((f.name, f.log, len(f.log) // 2))
    r = recycling()
    out.append((r.name, r.log, r.facts["cut"]))
    return [(n, log, k, oracle(log[:k]).snapshot_json()) for n, log, k in out]


# fragmented(n) for these n: 1 367 / 323 / 269 row segments at the end, which an MI355X holds in 298 /
# 72 / 61 leaf blocks at most (DocRes.max_lb): past the LDS plan's 128, and either side of 64
FRAG_SIZES = (1400, 350, 300)


# spliced(*a) for these: 700 appended rows, which an MI355X holds in 175 leaf blocks of 4 (it has left the
# LDS plan before the first set: pass 1's prefix runs HBM-resident), and 560 rows inserted at random
# positions, 111 fuller blocks, LDS-resident through both passes (580 such rows, 114 blocks, left it)
SPLICED = ((700, 90, None), (560, 40, 3))


def all_docs():
    return [fragmented(n) for n in FRAG_SIZES] + [spliced(*a) for a in SPLICED] + \
        [handle_levels(), recycling(), many_writers(70), many_writers(40)]


def check_against_oracle(doc):
    """The closed forms equal the oracle's summary; returns (oracle, parsed summary)."""
    o = oracle(doc.log)
    s = json.loads(o.snapshot_json())
    if doc.want_grid is not None:
        assert grid(s) == doc.want_grid, doc.name
    if doc.want_handles is not None:
        assert handles(s) == doc.want_handles, doc.name
    if doc.want_tables is not None:
        assert tables(s) == doc.want_tables, doc.name
    if doc.want_cells is not None:
        assert blob_cells(s) == doc.want_cells, doc.name
    return o, s
