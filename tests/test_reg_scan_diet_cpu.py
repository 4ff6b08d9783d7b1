"""The row engine's critical-path shortcuts (reg_engine.hpp), CPU build, bit-exact against the oracle on
status, segment table and text: the heap pop fused with the popped segment's search (heap_pop_find) and
the sift path found lane-parallel (pop_fast), on the documents that also sized the two shortcuts that
were measured and not kept (a remove scanning its row once, pack's sibling scours decided row-wide;
DESIGN 3.12). The event counters of the statistics build (tools/rg_stats.py names them) show that each
document has the removes, pops and packs its case is about."""
import ctypes
import importlib.util
import os
import random
import subprocess

import numpy as np
import pytest

from fluidframework_amd import mte
from tests import regcpu
from tests.oplog import dumps, ins, msg, rem

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _names():
    spec = importlib.util.spec_from_file_location("rg_stats", os.path.join(_ROOT, "tools", "rg_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.NAMES


@pytest.fixture(scope="module")
def stats():
    """Routes tests.regcpu through the statistics build; stats(fn) runs fn and returns the event counts
    of the replays it made (plus heap_max_at_pop), the oracle comparison included in fn."""
    nat = os.path.join(_ROOT, "tests", "native")
    base = regcpu.lib()
    subprocess.run(["make", "-s", "-C", nat, "stats"], check=True)
    L = ctypes.CDLL(os.path.join(nat, "_build", "libregcpu_stats.so"))
    for f in ("regcpu_replay", "regcpu_replay_paged", "regcpu_replay_props", "regcpu_replay_split", "regcpu_heap"):
        getattr(L, f).restype = getattr(base, f).restype
        getattr(L, f).argtypes = getattr(base, f).argtypes
    L.regcpu_docres_size.restype = ctypes.c_uint32
    L.regcpu_stats.restype = ctypes.c_uint32
    names = _names()

    def run(fn):
        out = (ctypes.c_uint64 * (len(names) + 2))()
        L.regcpu_stats(out, len(names) + 2)  # clear
        regcpu._lib = L
        try:
            fn()
        finally:
            regcpu._lib = base
        assert L.regcpu_stats(out, len(names) + 2) == len(names), "tools/rg_stats.py NAMES and RgStat differ"
        st = {k: int(out[i]) for i, k in enumerate(names)}
        st["heap_max_at_pop"] = int(out[len(names)])
        return st

    yield run
    regcpu._lib = base


# ---------------------------------------------------------------- generated documents


@pytest.mark.parametrize("n_ops", [3000, 20_000])
def test_kind2_eight_writers(stats, n_ops):
    """Kind 2, 8 writers: 3 000 ops reach a second row, 20 000 several (removes across rows, block splits
    inside a remove). Lean and paged engines."""
    ops, pay = regcpu.generated(2, 1000 + n_ops, n_ops, n_clients=8, seed=1000)

    def go():
        r = regcpu.compare(ops, pay)
        assert int(r["max_lb"]) > (8 if n_ops == 3000 else 24)
        regcpu.compare(ops, pay, pool_rows=32)

    st = stats(go)
    assert st["rem"] > 0 and st["rem_same_row_no_blk_split"] > 0 and st["pop"] > 0
    assert st["pack"] > 0 and st["pack_scour"] > st["pack_scour_nop"] > 0
    if n_ops == 20_000:
        assert st["rem_same_row"] < st["rem"]  # removes whose p2 lies in a later row
        assert st["rem_same_row_no_blk_split"] < st["rem_same_row"]  # block splits inside a remove
        assert st["range_rows"] > st["rem"] and st["res2_rows"] > st["rem"]  # markings, resolves over several rows


def test_gpu_case_heap_passes_64_entries(stats):
    """The 3 000-op kind-2 document of tests/test_gpu_scan_diet.py pops from a heap of more than 64
    entries (the sift path then runs into the second heap register)."""
    ops, pay = regcpu.generated(2, 1, 3000, n_clients=8, seed=17)
    st = stats(lambda: regcpu.compare(ops, pay))
    assert st["heap_max_at_pop"] > 64, st["heap_max_at_pop"]
    assert st["pack"] > 0 and st["split_blk"] > 0 and st["rem"] > 0


@pytest.mark.parametrize("wide", [False, True])
def test_kind3_ties_overlaps_annotates(stats, wide):
    """Kind 3 at 5 000 ops: forced ties (the `seen` rule), overlapping removes (F_OVL) and annotates on
    the PROPS engine, fixed rows and paged, and its WIDE form."""
    ops, pay = regcpu.generated(3, 7, 5000, n_clients=8, seed=1000)

    def go():
        regcpu.compare_props(ops, pay, wide=wide)
        regcpu.compare_props(ops, pay, pool_rows=32, wide=wide)

    st = stats(go)
    assert st["rem"] > 0 and st["pack"] > 0 and st["pop"] > 0


def test_wide_writers_above_32(stats):
    """33 writers and more: removers 32..63 (the second removers word)."""
    ops, pay = regcpu.generated(2, 3, 1200, n_clients=48, seed=1000)
    st = stats(lambda: regcpu.compare_props(ops, pay, wide=True))
    assert st["rem"] > 0 and st["pop"] > 0


# ---------------------------------------------------------------- built logs


def _builder_ops(msgs):
    b = mte.Builder()
    b.add_doc(dumps(msgs))
    batch = b.batch()
    ops = mte.batch_ops(batch).copy()
    n_pay = batch.doc_payload_offsets[1]
    pay = np.ctypeslib.as_array(batch.payload, shape=(max(n_pay, 1),))[:n_pay].copy()
    cno = batch.client_name_offsets
    names = [ctypes.string_at(batch.client_names + cno[i], cno[i + 1] - cno[i]).decode()
             for i in range(batch.doc_client_offsets[1])]
    return ops, pay, names


def _appended(n_segs, seg_len=10):
    """One writer appends n_segs segments of seg_len characters; the MSN stays 0, so nothing is ever
    scoured or merged: n_segs segments in document order, 4..7 per leaf block."""
    return [msg("a", i + 1, i, ins(i * seg_len, chr(ord("a") + i % 26) * seg_len), 0) for i in range(n_segs)]


def _run(stats, msgs):
    ops, pay, names = _builder_ops(msgs)
    return stats(lambda: regcpu.compare(ops, pay, names=names))


@pytest.mark.parametrize("n_segs,expect", [(4, "none"), (5, "none"), (6, "p2"), (7, "p1")])
def test_remove_inside_one_segment_at_the_block_limit(stats, n_segs, expect):
    """p1 and p2 inside the first segment of a block of n children: two splits in one block. From 5
    children the block ends at 7; from 6 the p2 split is the one that reaches 8 children and splits the
    block, from 7 the p1 split (p2 is then resolved over the moved blocks)."""
    st = _run(stats, _appended(n_segs) + [msg("b", n_segs + 1, n_segs, rem(3, 6), 0)])
    assert st["rem"] == 1 and st["split_at"] == 2
    assert st["rem_same_row"] == 1
    if expect == "none":
        assert st["rem_same_row_no_blk_split"] == 1 and st["split_blk"] == 0
    else:
        assert st["rem_same_row_no_blk_split"] == 0 and st["split_blk"] == 1


@pytest.mark.parametrize("p1,p2", [(10, 20), (0, 10), (10, 30), (20, 20)])
def test_remove_on_segment_boundaries_splits_nothing(stats, p1, p2):
    """p1 and p2 on existing segment boundaries (p1 == p2 too): no split."""
    st = _run(stats, _appended(5) + [msg("b", 6, 5, rem(p1, p2), 0)])
    assert st["split_at"] == 0 and st["rem_same_row_no_blk_split"] == 1


def test_remove_across_a_row_boundary(stats):
    """80 appended segments fill more than 8 leaf blocks; a remove from the middle of the first row to the
    middle of the second resolves p2 and marks row by row (twice, the second over the first's
    tombstones); one stays inside the first row."""
    n = 80
    msgs = _appended(n) + [msg("b", n + 1, n, rem(205, 555), 0), msg("c", n + 2, n, rem(5, 25), 0),
                           msg("b", n + 3, n + 2, rem(100, 500), 0)]
    ops, pay, names = _builder_ops(msgs)
    st = stats(lambda: regcpu.compare(ops, pay, names=names))
    at, res, _, _ = regcpu.replay(ops, pay)
    assert int(res["n_lb"]) > 8
    assert st["rem"] == 3 and st["rem_same_row"] == 1 and st["range_rows"] >= 5 and st["res2_rows"] >= 5


@pytest.mark.parametrize("seed", range(3))
def test_long_segments_among_packed_siblings(stats, seed):
    """Segments longer than 256 units: blocks that take the serial scour are among the siblings pack
    re-scours (they can change on a second pass)."""
    from oracle import OracleDoc

    rng = random.Random(300 + seed)
    d = OracleDoc()
    msgs, refs, seq, order = [], {c: 0 for c in "abc"}, 0, []
    for _ in range(1500):
        c = rng.choice("abc")
        refs[c] = rng.randint(max(refs[c], seq - 6), seq)
        if c not in order:
            order.append(c)
        L = d.length_at(refs[c], order.index(c) + 1)
        if L == 0 or rng.random() < 0.5:
            n = rng.choice([1, 2, 5, 40, 250, 257, 300, 600])
            contents = ins(rng.randint(0, L), "".join(rng.choice("xyz") for _ in range(n)))
        else:
            a = rng.randint(0, L - 1)
            contents = rem(a, min(L, a + rng.randint(1, 400)))
        seq += 1
        m = msg(c, seq, refs[c], contents, min(refs.values()))
        msgs.append(m)
        d.apply_json(dumps([m]))
    st = _run(stats, msgs)
    assert st["scour_serial"] > 0 and st["pack"] > 0 and st["pack_scour"] > st["pack_scour_nop"] > 0


@pytest.mark.parametrize("seed", range(4))
def test_concurrent_writers_ties_and_overlaps(stats, seed):
    """Five writers with stale reference sequence numbers: zero-length ties at p1 and p2 (tombstones seen
    or not at the refSeq), overlapping removes, markers."""
    from oracle import OracleDoc

    rng = random.Random(40 + seed)
    d = OracleDoc()
    msgs, refs, seq, order = [], {c: 0 for c in "abcde"}, 0, []
    for _ in range(1500):
        c = rng.choice("abcde")
        refs[c] = rng.randint(max(refs[c], seq - 12), seq)
        if c not in order:
            order.append(c)
        L = d.length_at(refs[c], order.index(c) + 1)
        if L == 0 or rng.random() < 0.4:
            seg = {"marker": {"refType": rng.choice([0, 1, 2])}} if rng.random() < 0.15 else \
                "".join(rng.choice("pq") for _ in range(rng.randint(1, 5)))
            contents = ins(rng.randint(0, L), seg)
        else:
            a = rng.randint(0, L - 1)
            contents = rem(a, min(L, a + rng.randint(1, 9)))
        seq += 1
        m = msg(c, seq, refs[c], contents, min(refs.values()))
        msgs.append(m)
        d.apply_json(dumps([m]))
    st = _run(stats, msgs)
    assert st["rem"] > 500 and st["rem_same_row"] > 100
