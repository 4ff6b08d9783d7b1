"""Log builders for tests/test_gpu_emit_edges.py: documents whose final segment table hands emission
(emit.hip) unmerged rows at the sizes where its code paths change, each with the precondition that
keeps it from going vacuous.

Zamboni merges settled neighbours itself, so these logs are "lazy": every insert / remove carries
MSN 0 and one tail op (an empty remove) carries the MSN up. Zamboni then reaches only the first few
blocks, and the rows behind them arrive at emission one per insert, all settled. A case is
(name, log, check); check(Shape) asserts the shape that makes the case meaningful on the oracle's
JSON path and returns a line saying what it asserted."""
import json

from oracle import OracleDoc
from tests.oplog import ann, ins, msg, rem

HI, LO = "\ud83d", "\ude00"  # U+1F600 as a split pair
PAT = 'a"é\u0001b\\漢\t'    # 1-, 2-, 3- and 6-byte JSON forms


def units(s):
    return len(s.encode("utf-16-le", "surrogatepass")) // 2


def norm(s):
    """Adjacent surrogate halves as the one character JSON parsing makes of them."""
    return s.encode("utf-16-le", "surrogatepass").decode("utf-16-le", "surrogatepass")


def pat(n, at=0):
    return "".join(PAT[(at + i) % len(PAT)] for i in range(n))


def put(s, i, t):
    """s with the units from i on replaced by t (BMP text only)."""
    return s[:i] + t + s[i + len(t):]


class Lazy:
    """One writer appending rows; nothing settles before tail()."""

    def __init__(self, writer="w0"):
        self.msgs, self.seq, self.len, self.writer = [], 0, 0, writer

    def op(self, contents, msn=0, writer=None):
        self.seq += 1
        self.msgs.append(msg(writer or self.writer, self.seq, self.seq - 1, contents, msn))
        return self.seq

    def add(self, text, props=None, writer=None, at=None):
        """A text row at the end (or at unit `at`, a row boundary); returns its first unit."""
        pos = self.len if at is None else at
        self.op(ins(pos, {"text": text, "props": props} if props else text), writer=writer)
        self.len += units(text)
        return pos

    def marker(self, props=None, at=None):
        seg = {"marker": {"refType": 1}}
        if props:
            seg["props"] = props
        pos = self.len if at is None else at
        self.op(ins(pos, seg))
        self.len += 1
        return pos

    def fill(self, n, ch="x"):
        for _ in range(n):
            self.add(ch)

    def remove(self, a, b, writer=None):
        self.op(rem(a, b), writer=writer)
        self.len -= b - a

    def annotate(self, a, b, props):
        self.op(ann(a, b, props))

    def trail(self):
        """Trailing filler with a marker after every tenth row, so that small chunks close often."""
        for _ in range(7):
            self.fill(10, "y")
            self.marker()

    def tail(self, msn=None):
        """The op that carries the MSN: everything at or below it settles."""
        self.op(rem(0, 0), msn=self.seq if msn is None else msn)
        return self.msgs


# with one tail op zamboni merges the first 16 one-unit rows into 4: a row inserted after `k >= 16`
# one-unit rows ends up at table row k - LEAD (every check below asserts where its rows landed)
LEAD = 12


class Shape:
    """What the oracle's JSON path makes of a log: the segment table and the parsed SnapshotV1."""

    def __init__(self, log, chunk=10000):
        o = OracleDoc()
        text = json.dumps(log)
        o.apply_json(text)
        assert o.status()[0] == 0, o.status()
        self.oracle = o
        self.segs = json.loads(o.segments_json())
        self.blobs = [json.loads(e["value"]["contents"]) for e in json.loads(o.snapshot_json(chunk))["entries"]]
        self.min_seq = self.blobs[0]["headerMetadata"]["minSequenceNumber"]
        self.entries = [x for b in self.blobs for x in b["segments"]]

    def settled(self, i):
        s = self.segs[i]
        return s["seq"] <= self.min_seq and "removedSeq" not in s

    def elided(self, i):
        s = self.segs[i]
        return "removedSeq" in s and s["removedSeq"] <= self.min_seq

    def row(self, text):
        """The one table row with this text."""
        k = [i for i, s in enumerate(self.segs) if s["kind"] == "T" and s["text"] == norm(text)]
        assert len(k) == 1, (text, k)
        return k[0]

    def rows_of(self, texts):
        """Consecutive table rows with these texts; the first one's index."""
        k = self.row(texts[0])
        assert [s.get("text") for s in self.segs[k: k + len(texts)]] == [norm(t) for t in texts], k
        return k

    @staticmethod
    def entry_text(x):
        if isinstance(x, str):
            return x
        if "json" in x:
            return Shape.entry_text(x["json"])
        return x.get("text")  # None: a marker

    def entry_with(self, text):
        """Index of the one snapshot entry whose text contains `text`."""
        k = [i for i, x in enumerate(self.entries) if norm(text) in (self.entry_text(x) or "")]
        assert len(k) == 1, (text, k)
        return k[0]

    def entry_rows(self, e):
        """Table rows [first, last] of settled text entry e: entries and unelided rows in step."""
        want = self.entry_text(self.entries[e])
        at = 0
        for i, x in enumerate(self.entries[:e]):
            at = self._skip(at, x)
        first = at
        while self.elided(first):
            first += 1
        got, last = "", first - 1
        while units(got) < units(want):
            last += 1
            if not self.elided(last):
                got += self.segs[last]["text"]
        assert _same(got, want), (got, want)
        return first, last

    def _skip(self, at, x):
        want = self.entry_text(x)
        n = 1 if want is None else units(want)
        got = 0
        while got < n:
            if not self.elided(at):
                got += self.segs[at]["len"]
            at += 1
        return at


def _same(a, b):
    enc = lambda s: s.encode("utf-16-le", "surrogatepass")  # noqa: E731 (a joined pair = its two halves)
    return enc(a) == enc(b)


# ------------------------------------------------------------------------------------------- a
A_SIZES = (31, 32, 33, 64)


def _a_rows(flavour):
    rows = []
    for n in A_SIZES:
        if flavour == "ascii":
            t = ("abcdefghij" * 7)[:n]
        elif flavour == "quotes":
            t = '"' * n
        elif flavour == "ctl":
            t = "\u0001" * n
        elif flavour == "ends_hi":
            t = pat(n - 1, n) + HI
        elif flavour == "starts_lo":
            t = LO + pat(n - 1, n)
        elif flavour == "pair":  # a whole pair on units 31/32 (the last two units of the shorter rows)
            k = 31 if n >= 33 else n - 2
            t = pat(k, n) + HI + LO + pat(n - k - 2, n + 1)
        else:  # "hi_lo": every row ends in a high surrogate and the next starts with the low one
            t = (LO if rows else "q") + pat(n - 2, n) + HI
        assert units(t) == n
        rows.append(t)
    if flavour == "hi_lo":
        rows.append(LO + "z")
    return rows


def case_a(flavour):
    d = Lazy()
    d.fill(30)
    rows = _a_rows(flavour)
    for t in rows:
        d.add(t)
    d.trail()
    log = d.tail()

    def check(s):
        k = s.rows_of(rows)
        assert k == 30 - LEAD and all(s.settled(k + i) for i in range(len(rows)))
        assert [s.segs[k + i]["len"] for i in range(4)] == list(A_SIZES)
        e = s.entry_with(rows[0][:8])
        assert s.entry_rows(e)[0] < k and s.entry_rows(e)[1] > k + 3  # one run over all of them
        return f"rows {k}..{k + 3} are {A_SIZES} units ({flavour}), settled, inside one header entry"

    return f"a_{flavour}", log, check


# ---------------------------------------------------------------------------------------- b, c
BC_SIZES = (65, 128, 129, 200)


def case_bc(kind):
    d = Lazy()
    d.fill(30)
    rows = []
    if kind in ("pair63", "hi63", "lo64", "pair127"):
        # each row twice: behind a marker, where it starts an entry (WRITE's 64-unit steps count from
        # the entry's first unit), and inside a run (COUNT's count from the row's)
        for off in (0, 1):
            for n in BC_SIZES:
                t = pat(n, n + off)
                if kind == "pair63":
                    t = put(t, 63, HI + LO)
                elif kind == "hi63":
                    t = put(t, 63, HI)
                elif kind == "lo64":
                    t = put(t, 64, LO)
                elif n > 128:
                    t = put(t, 127, HI + LO)
                else:
                    continue
                assert units(t) == n
                rows.append(t)
                if off == 0:
                    d.marker()
                d.add(t)
                d.fill(2)
    else:  # "end_hi": rows of exactly 64 and 128 units ending in a high surrogate, then only the low one
        for off in (0, 1):
            for n in (64, 128):
                rows.append(pat(n - 1, n + off) + HI)
                if off == 0:
                    d.marker()
                d.add(rows[-1])
                d.add(LO)
                d.fill(2)
    d.fill(70, "y")
    log = d.tail()

    def check(s):
        if kind == "end_hi":
            ks = [s.row(t) for t in rows]
            for k, t in zip(ks, rows):
                assert s.segs[k]["len"] == units(t) and s.segs[k + 1]["text"] == LO and s.settled(k) and s.settled(k + 1)
            assert [s.segs[k - 1]["kind"] for k in ks] == ["M", "M", "T", "T"]
            txt = [s.entry_text(x) or "" for x in s.entries]
            assert sum(t.count("\U0001F600") for t in txt) == 4 and not any(HI in t or LO in t for t in txt)
            return (f"rows {ks} are 64 / 128 / 64 / 128 units ending in a high surrogate, each next row is the low "
                    f"one alone; the first two start an entry, the others sit inside a run; all four pairs join")
        ks = [s.row(t) for t in rows]
        assert all(s.settled(k) and s.segs[k]["len"] == units(t) for k, t in zip(ks, rows))
        half = len(rows) // 2
        assert all(s.segs[k - 1]["kind"] == "M" for k in ks[:half])
        assert all(s.segs[k - 1]["kind"] == "T" and s.settled(k - 1) for k in ks[half:])
        for t in rows:
            u = t.encode("utf-16-le", "surrogatepass")
            at = {"pair63": 63, "hi63": 63, "lo64": 64, "pair127": 127}[kind]
            assert 0xD800 <= int.from_bytes(u[2 * at: 2 * at + 2], "little") <= 0xDFFF
        return (f"rows {ks} are single inserts of {[units(t) for t in rows]} units, settled ({kind}), "
                f"the first {half} each behind a marker, the others inside a run")

    return f"bc_{kind}", log, check


# ------------------------------------------------------------------------------------------- d
def case_d(hi_row, between=None):
    """One-unit rows with a split pair on table rows hi_row / hi_row + 1 (between None), or with a
    marker / a segment above minSeq ("info") on the row between its halves."""
    d = Lazy()
    d.fill(hi_row + LEAD)
    d.add(HI)
    if between == "marker":
        d.marker()
    at = d.len
    d.add(LO)
    d.trail()
    msn = None
    if between == "info":
        msn = d.seq
        d.add("I", at=at)
    log = d.tail(msn)

    def check(s):
        k = s.row(HI)
        assert k == hi_row and s.settled(k)
        lo = k + (2 if between else 1)
        assert s.segs[lo]["text"] == LO and s.settled(lo)
        if between is None:
            e = s.entry_with("\U0001F600")
            f, l = s.entry_rows(e)
            assert f < 60 and l > 66 and len(s.segs) > 130
            return f"the pair is on rows {k}/{lo}, inside the run of rows {f}..{l} that forms entry {e}"
        mid = s.segs[k + 1]
        if between == "marker":
            assert mid["kind"] == "M" and s.settled(k + 1)
        else:
            assert mid["text"] == "I" and mid["seq"] > s.min_seq
            assert "json" in s.entries[s.entry_with("I")]
        e = s.entry_with(HI)
        assert s.entry_rows(e)[1] == k and s.entry_text(s.entries[e + 2]).startswith(LO)
        return f"high surrogate on row {k}, {between} on row {k + 1}, low surrogate on row {lo}: the run ends on row {k}"

    return f"d_{hi_row}_{between or 'pair'}", log, check


# ------------------------------------------------------------------------------------------- e
def case_e(name, sizes, want):
    """Adjacent settled rows of `sizes` units between two markers; `want`: the entries' lengths."""
    d = Lazy()
    d.fill(30)
    d.marker()
    rows = [pat(n, 3 * i) for i, n in enumerate(sizes)]
    for t in rows:
        d.add(t)
    d.marker()
    d.fill(70, "y")
    log = d.tail()

    def check(s):
        k = s.rows_of(rows)
        assert all(s.settled(k + i) for i in range(len(rows)))
        assert s.segs[k - 1]["kind"] == "M" and s.segs[k + len(rows)]["kind"] == "M"
        m = [i for i, x in enumerate(s.entries) if s.entry_text(x) is None]
        assert len(m) == 2
        got = [units(s.entry_text(x)) for x in s.entries[m[0] + 1: m[1]]]
        assert got == want, got
        return f"rows {k}..{k + len(rows) - 1} of {sizes} units, settled, form entries of {want}"

    return f"e_{name}", log, check


# ------------------------------------------------------------------------------------------- f
def case_f(hi_row, gaps):
    """High surrogate, elided text rows of `gaps` units each, low surrogate."""
    d = Lazy()
    d.fill(hi_row + LEAD)
    d.add(HI)
    a = d.len
    gone = [pat(n, 5 + i) if n > 1 else "QR"[i] for i, n in enumerate(gaps)]
    for t in gone:
        d.add(t)
    b = d.len
    d.add(LO)
    d.trail()
    d.remove(a, b)
    log = d.tail()

    def check(s):
        k = s.row(HI)
        assert k == hi_row and s.settled(k)
        for i, t in enumerate(gone):
            assert s.segs[k + 1 + i]["text"] == t and s.elided(k + 1 + i)
        lo = k + 1 + len(gone)
        assert s.segs[lo]["text"] == LO and s.settled(lo)
        e = s.entry_with("\U0001F600")
        f, l = s.entry_rows(e)
        assert f < k and l > lo
        return f"row {k} high surrogate, rows {k + 1}..{lo - 1} ({gaps} units) removed at or below minSeq {s.min_seq}, row {lo} low surrogate; one entry"

    return f"f_{hi_row}_{'_'.join(map(str, gaps))}", log, check


# ------------------------------------------------------------------------------------------- g
def case_g(props):
    d = Lazy()
    for _ in range(30):
        d.add("x", props)
    rows = ["mid\ndle", "cd", "ab\n", "ef", "gh\n", "ij"]
    for t in rows[:5]:
        d.add(t, props)
    d.add("", props)  # accepted, and makes no row
    d.add(rows[5], props)
    for _ in range(70):
        d.add("y", props)
    log = d.tail()

    def check(s):
        k = s.rows_of(rows)
        assert all(s.settled(k + i) for i in range(6)) and not any(x["len"] == 0 for x in s.segs)
        if props:
            assert all(json.loads(x["props"]) == props for x in s.segs[k: k + 6])
        txt = [s.entry_text(x) for x in s.entries]
        e = s.entry_with("mid\ndle")
        assert txt[e].endswith("xmid\ndlecdab\n") and txt[e + 1] == "efgh\n" and txt[e + 2].startswith("ijyy")
        return (f"rows {k}..{k + 5}: a row with a newline inside joins, the rows after 'ab\\n' and 'gh\\n' start "
                f"entries {e + 1} and {e + 2} (an empty insert after 'gh\\n' leaves no row){' with props' if props else ''}")

    return f"g_{'props' if props else 'plain'}", log, check


# ------------------------------------------------------------------------------------------- h
H_CHUNKS = (1, 5, 64, 257)


def case_h():
    """Entries that end exactly on a chunk of 5, 64 and 257: 5 | marker, 58 | marker, 191, marker."""
    d = Lazy()
    d.add("abcde")
    d.marker()
    d.add(pat(58))
    d.marker()
    d.add(pat(191, 2))
    d.marker()
    d.trail()
    for _ in range(3):
        d.fill(90, "z")
        d.marker()
    log = d.tail()

    def check(s):
        lens, at = [], 0
        for x in s.entries:
            t = s.entry_text(x)
            at += 1 if t is None else units(t)
            lens.append(at)
        assert all(c in lens for c in H_CHUNKS[1:]), lens
        for c in H_CHUNKS:
            n = len(Shape(log, c).blobs)
            assert n >= 3, (c, n)
        return f"entries end at lengths {lens[:6]}: exactly on chunks of 5, 64 and 257"

    return "h_exact", log, check


# ------------------------------------------------------------------------------------------- i
I_KEYS = ["10", "9", "0", "4294967294", "4294967295", "01", "-1", "1.5", "b"]


def case_i_keys():
    d = Lazy()
    d.fill(30)
    a = d.add("prop")
    d.fill(70, "y")
    for i, k in enumerate(I_KEYS):
        d.annotate(a, a + 4, {k: [i, "v", True, {"z": 1}][i % 4]})
    log = d.tail()

    def check(s):
        k = s.row("prop")
        keys = list(json.loads(s.segs[k]["props"]))
        assert keys == ["0", "9", "10", "4294967294", "4294967295", "01", "-1", "1.5", "b"], keys
        e = s.entries[s.entry_with("prop")]
        assert list(e["props"]) == keys
        return f"row {k} carries {keys}: array-index keys ascending, then the others in insertion order"

    return "i_keys", log, check


def case_i_map(n):
    """Rows whose maps hold n keys (7 fills the narrow map record, 8 needs the wide one)."""
    d = Lazy()
    d.fill(30)
    p = {f"k{i}": i for i in range(n)}
    a = d.add("full", p)
    d.add("more", dict(reversed(list(p.items()))))  # the same map in another order: joins
    d.add("less", {f"k{i}": i for i in range(n - 1)})
    d.fill(70, "y")
    d.annotate(a + 8, a + 12, {f"k{n - 1}": n - 1})  # "less" grows to the same n keys, last
    log = d.tail()

    def check(s):
        k = s.rows_of(["full", "more", "less"])
        assert all(len(json.loads(s.segs[k + i]["props"])) == n for i in range(3))
        e = s.entries[s.entry_with("full")]
        assert e["text"] == "fullmoreless" and len(e["props"]) == n
        return f"rows {k}..{k + 2} carry maps of {n} keys in three insertion orders and form one entry"

    return f"i_map{n}", log, check


# ------------------------------------------------------------------------------------------- j
J_NAMES = ['w"1', "é\\", "\u0001", "n" * 40]


def case_j():
    d = Lazy()
    d.fill(100)
    msn = d.seq
    for i, w in enumerate(J_NAMES):
        d.add("ABCD"[i] * 3, writer=w, at=40 + 10 * i)
    d.remove(90, 91, writer=J_NAMES[0])
    log = d.tail(msn)

    def check(s):
        info = [x for x in s.entries if not isinstance(x, str) and "json" in x]
        assert [x.get("client") for x in info[:4]] == J_NAMES and info[4]["removedClient"] == J_NAMES[0]
        assert all(x["seq"] > s.min_seq for x in info[:4])
        return f"merge-info entries carry the clients {J_NAMES!r} and a removedClient, all above minSeq {s.min_seq}"

    return "j_names", log, check


def all_cases():
    c = [case_a(f) for f in ("ascii", "quotes", "ctl", "ends_hi", "starts_lo", "pair", "hi_lo")]
    c += [case_bc(k) for k in ("pair63", "pair127", "hi63", "lo64", "end_hi")]
    c += [case_d(r) for r in (62, 63, 64)]
    c += [case_d(r, b) for b in ("marker", "info") for r in (62, 63)]
    c += [case_e("256_257", (256, 257), [513]), case_e("257_256", (257, 256), [513]),
          case_e("257_257", (257, 257), [257, 257]), case_e("258_then_257", (200, 57, 1, 257), [258, 257]),
          case_e("258_then_256", (200, 57, 1, 256), [514]), case_e("257_then_257", (200, 56, 1, 257), [257, 257])]
    c += [case_f(30, (1,)), case_f(63, (1,)), case_f(62, (1, 1)), case_f(30, (40,)), case_f(63, (40,))]
    c += [case_g(None), case_g({"b": 1})]
    c += [case_h(), case_i_keys(), case_i_map(7), case_i_map(8), case_j()]
    return c


def chunk_cases():
    """Case h's documents: those of a, d and f, and the one whose entries end on the chunks."""
    return [x for x in all_cases() if x[0][0] in "adfh"]


# --------------------------------------------------------------- object values beyond 64 a batch
def object_value_docs(n_distinct=70):
    """Logs for one batch: documents that intern n_distinct distinct object values first, then pairs
    of adjacent settled rows whose maps differ only in an object value that matchProperties calls
    equal (and one that it does not), once with the MSN following the seq (zamboni decides) and once
    lazy (emission decides). Returns (logs, checks): checks[i](Shape) for logs[i], or None."""
    logs, checks = [], []
    for half in range(2):  # two documents share the distinct values
        d = Lazy()
        d.fill(n_distinct // 2, "v")
        for i in range(n_distinct // 2):
            d.annotate(i, i + 1, {"k": {"n": half * (n_distinct // 2) + i}})
        logs.append(d.tail())
        checks.append(None)
    pairs = [("same_keys", {"k": {"a": 1, "b": 2}}, {"k": {"b": 2, "a": 1}}, True),
             ("array", {"k": [1, 2]}, {"k": {"0": 1, "1": 2}}, True),
             ("control", {"k": {"a": 1, "b": 2}}, {"k": {"a": 1, "b": 3}}, False)]
    for name, pa, pb, joins in pairs:
        for lazy in (False, True):
            d = Lazy()
            if lazy:
                d.fill(30)
                d.add("ab", pa)
                d.add("cd", pb)
                d.fill(70, "y")
                log = d.tail()
            else:  # the MSN follows the seq
                for t, p in (("xx", None), ("ab", pa), ("cd", pb), ("yy", None), ("zz", None)):
                    d.seq += 1
                    d.msgs.append(msg("w0", d.seq, d.seq - 1, ins(d.len, {"text": t, "props": p} if p else t), d.seq - 1))
                    d.len += 2
                log = d.tail()
                log = d.tail()

            def check(s, joins=joins, lazy=lazy, name=name):
                txt = [s.entry_text(x) for x in s.entries]
                if joins:
                    assert "abcd" in txt and "ab" not in txt, txt
                else:
                    assert "ab" in txt and "cd" in txt, txt
                rows = [x["text"] for x in s.segs]
                if lazy:  # emission coalesces: the table still has both rows
                    assert "ab" in rows and "cd" in rows
                elif joins:  # zamboni did
                    assert "abcd" in rows
                return f"{name}, {'lazy' if lazy else 'msn follows seq'}: {'one entry' if joins else 'two entries'}"

            logs.append(log)
            checks.append(check)
    return logs, checks


def object_limit_log(pairs):
    """`pairs` pairs of adjacent settled rows "pNN" / "qNN" whose maps hold the same object in two key
    orders: 2 * pairs object values that each equal another one."""
    d = Lazy()
    d.fill(30)
    for i in range(pairs):
        d.add(f"p{i:02d}", {"k": {"a": i, "b": 1}})
        d.add(f"q{i:02d}", {"k": {"b": 1, "a": i}})
    d.fill(70, "y")
    return d.tail()
