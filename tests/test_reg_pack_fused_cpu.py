"""The row engine's pack path (reg_engine.hpp zamboni / pack_leaves) and the needsScour marks an edit
folds into its own row write (the engines with a whole row store: k_solo's; not k_rows'), CPU build, bit-exact against the oracle on status, segment table and text.
The sibling pass of a pack scours the popped block a second time, and that call is NOT a no-op: a
tombstone the first pass dropped had reset the merge chain, so the settled text on its two sides joins
only in the second pass (pack_self_changed counts those; an engine that skips the call differs from the
oracle from op 859 of C4's longest document on). The other pack counters (tools/rg_stats.py names them)
show that the documents meet the shapes a pack can take: siblings in two rows, more blocks out than
siblings in, cascades into pack_internal, a sibling on the serial walk.

What a fused pack (decide per sibling, gather by keep mask) would have to fall back on is
sized here too: packs with a sibling on the serial walk or with an arena_gc during the pass are at most
5 % of the packs of C4's longest document. The CPU harness sizes the arena from the payload
(tests/regcpu.py), which no document of this file fills: an arena_gc inside a pack does not occur here."""
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
    """Routes tests.regcpu through the statistics build; stats(fn) runs fn (the oracle comparison in it)
    and returns the event counts of the replays it made."""
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
        assert st["pack_one_row"] + st["pack_two_rows"] == st["pack"], st  # every pack was shaped
        assert st["pack_self_changed"] <= st["pack"], st
        return st

    yield run
    regcpu._lib = base


def test_c4_longest_document_prefix(stats):
    """The first 200 000 ops of C4's longest document (kind 2, global id 111877): every pack shape but
    the serial walk, which this document never takes; the packs a fused pack would hand back to the
    per-sibling path are at most 5 % (none: no serial sibling, no arena_gc inside a pack)."""
    ops, pay = regcpu.generated(2, 111877, 200_000, n_clients=8, seed=1000)
    st = stats(lambda: regcpu.compare(ops, pay))
    assert st["ops"] == 200_000 and st["pack"] > 10_000
    assert st["pack_two_rows"] > 0 and st["pack_one_row"] > 0
    assert st["pack_grows"] > 0 and st["pack_cascade"] > 0
    assert st["pack_m8"] == 0  # a level-1 node splits on reaching 8 children: a pack sees 7 siblings at most
    assert st["scour_serial"] == 0
    assert st["pack_serial"] + st["pack_gc"] <= 0.05 * st["pack"], st
    assert st["pack_sib_changed"] > st["pack"]  # more than one changed sibling per pack
    assert st["pack_self_changed"] > 0  # the popped block's second scour joins across a dropped tombstone
    # the needsScour marks of inserts and removes ride on the edit's row write; the ones left are
    # the inserts whose block split
    assert st["lru_folded"] > st["lru_rewrite"] > 0, st
    assert st["lru_folded"] + st["lru_rewrite"] == st["lru_push"]


def test_kind5_continuous_zamboni(stats):
    """Kind 5 (MSN lag <= 64): zamboni after nearly every op, small heap, packs all the time."""
    ops, pay = regcpu.generated(5, 29, 20_000, n_clients=8, seed=1000)

    def go():
        regcpu.compare(ops, pay)
        regcpu.compare(ops, pay, pool_rows=32)

    st = stats(go)
    assert st["pack"] > 1000 and st["pack_two_rows"] > 0 and st["pack_cascade"] > 0
    assert st["lru_folded"] > 0


@pytest.mark.parametrize("clients", [8, 31])
@pytest.mark.parametrize("pool", [0, 32])
def test_kind3_joins_by_properties(stats, clients, pool):
    """Kind 3 (properties, annotates, ties): the joins of a scour depend on match_props; fixed rows and
    the paged pool."""
    ops, pay = regcpu.generated(3, 7 + clients, 5000, n_clients=clients, seed=1000)
    st = stats(lambda: regcpu.compare_props(ops, pay, pool_rows=pool))
    assert st["pack"] > 0 and st["pack_sib_changed"] > 0 and st["lru_rewrite"] > 0
    # the marks are folded on the engines with a whole row store (k_solo's), not on the paged pool's
    assert (st["lru_folded"] > 0) == (pool == 0) and st["lru_folded"] + st["lru_rewrite"] == st["lru_push"], st


def test_wide_33_writers(stats):
    """33 writers on the WIDE engine (removers 32..63 in the second removers word)."""
    ops, pay = regcpu.generated(2, 3, 1200, n_clients=33, seed=1000)
    st = stats(lambda: regcpu.compare_props(ops, pay, wide=True))
    assert st["pack"] > 0 and st["rem"] > 0 and st["lru_folded"] > 0


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


@pytest.mark.parametrize("seed", range(2))
def test_serial_walk_inside_a_pack(stats, seed):
    """Inserts of 1..600 characters (as test_long_segments_granularity): packs whose siblings hold a
    joining slot of more than 256 units, which the sibling pass scours on the serial walk."""
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
    ops, pay, names = _builder_ops(msgs)
    st = stats(lambda: regcpu.compare(ops, pay, names=names))
    assert st["scour_serial"] > 0 and st["pack_serial"] > 0, st


@pytest.mark.parametrize("kind,n_ops,clients,gid,seed", [(2, 3000, 8, 1, 17), (3, 2000, 8, 7, 1000), (2, 1200, 33, 3, 1000),
                                                         (5, 2000, 8, 0, 1000)])
def test_gpu_cases_reach_the_pack_shapes(stats, kind, n_ops, clients, gid, seed):
    """The documents of tests/test_gpu_pack_fused.py on the CPU build: each packs, the lean one with
    siblings in two rows and cascades into pack_internal, and every one folds needsScour marks."""
    ops, pay = regcpu.generated(kind, gid, n_ops, n_clients=clients, seed=seed)
    if kind == 3:
        st = stats(lambda: regcpu.compare_props(ops, pay, wide=True))
    elif clients > 32:
        st = stats(lambda: regcpu.compare_props(ops, pay, wide=True))
    else:
        st = stats(lambda: regcpu.compare(ops, pay))
    assert st["pack"] > 0 and st["lru_folded"] > 0, st
    if kind == 2 and clients == 8:
        assert st["pack_two_rows"] > 0 and st["pack_cascade"] > 0, st


@pytest.mark.parametrize("gid", [0, 1])
@pytest.mark.parametrize("kind,n_ops", [(2, 3000), (3, 2000), (5, 2000)])
def test_gpu_k_rows_documents_reach_the_pack_shapes(stats, kind, n_ops, gid):
    """The first two of the 48 documents tests/test_gpu_pack_fused.py replays on k_rows (the ones it
    compares in full), on the fixed rows and on the paged pool: each packs and folds marks; the kind-2
    ones grow past 8 leaf blocks (a second row, so the paged engine maps more than one pool row) and
    pack siblings that lie in two rows, with cascades into pack_internal."""
    ops, pay = regcpu.generated(kind, gid, n_ops, n_clients=8, seed=1000)
    res = []

    def go():
        for pool in (0, 32):
            res.append(regcpu.compare_props(ops, pay, pool_rows=pool) if kind == 3 else
                       regcpu.compare(ops, pay, pool_rows=pool or None))

    st = stats(go)
    assert st["pack"] > 0 and st["lru_folded"] > 0, st
    if kind == 2:
        assert all(int(r["max_lb"]) > 8 for r in res), [int(r["max_lb"]) for r in res]
        assert st["pack_two_rows"] > 0 and st["pack_cascade"] > 0, st
