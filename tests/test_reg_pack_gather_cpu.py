"""The fused pack (reg_engine.hpp pack_fused: every sibling of a pack decided at once from row-wide masks,
the kept slots gathered by keep mask) on the CPU build, against the oracle on status, segment table and
text, and against an unfused build of the same tree (tests/native/pack_gather.mk, MTE_FUSED_PACK=0) on the
DocRes arena_top / arena_sel / n_gc -- equal only when every fresh chunk was allocated in scour's order --
and on the sibling-pass counters, which keep their meaning on the fused path (siblings decided /
unchanged / changed). Every case asserts by counter (tools/rg_stats.py names them) that it reaches its
shape. The fused path is built into the engines that own a whole row store (k_solo's, k_rows_cont's: the
fixed-row CPU engines); the paged pool keeps the sibling loop and must count no fused pack."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from fluidframework_amd import mte
from tests import regcpu
from tests.oplog import dumps
from tests.pack_gather_docs import SOLO_DOCS, long_insert_log, tombstone_log

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NATIVE = os.path.join(_ROOT, "tests", "native")
# the arena of test_arena_gc_hands_the_pack_back: found on the CPU build by stepping down from the harness
# default (6 * payload + 4096 = 35 728 units). From 3 000 units down packs need an arena_gc; at 1 400 five
# of the 327 do and the document still replays (at 400 it fails with MTE_DOC_CAPACITY, as the oracle does not)
GC_ARENA_CAP = 1400


def _names():
    spec = importlib.util.spec_from_file_location("rg_stats", os.path.join(_ROOT, "tools", "rg_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.NAMES


@pytest.fixture(scope="module")
def both():
    """both(fn): fn() -- replays and oracle comparisons through tests.regcpu, returning DocRes records --
    on the statistics build and on its unfused twin. Asserts what the two must share, returns the fused
    build's counters."""
    base = regcpu.lib()
    subprocess.run(["make", "-s", "-C", _NATIVE, "stats"], check=True)
    subprocess.run(["make", "-s", "-C", _NATIVE, "-f", "pack_gather.mk", "_build/libregcpu_unfused.so"], check=True)
    names = _names()
    libs = []
    for so in ("libregcpu_stats.so", "libregcpu_unfused.so"):
        L = ctypes.CDLL(os.path.join(_NATIVE, "_build", so))
        for f in ("regcpu_replay", "regcpu_replay_paged", "regcpu_replay_props", "regcpu_replay_split", "regcpu_heap"):
            getattr(L, f).restype = getattr(base, f).restype
            getattr(L, f).argtypes = getattr(base, f).argtypes
        L.regcpu_docres_size.restype = ctypes.c_uint32
        L.regcpu_stats.restype = ctypes.c_uint32
        libs.append(L)

    def one(L, fn):
        out = (ctypes.c_uint64 * (len(names) + 2))()
        L.regcpu_stats(out, len(names) + 2)  # clear
        regcpu._lib = L
        try:
            res = fn()
        finally:
            regcpu._lib = base
        assert L.regcpu_stats(out, len(names) + 2) == len(names), "tools/rg_stats.py NAMES and RgStat differ"
        return res, {k: int(out[i]) for i, k in enumerate(names)}

    def run(fn):
        rf, sf = one(libs[0], fn)
        ru, su = one(libs[1], fn)
        for a, b in zip(rf, ru):
            for k in ("status", "arena_top", "arena_sel", "n_gc", "n_lb", "max_lb", "seg_next", "heap_size"):
                assert int(a[k]) == int(b[k]), (k, int(a[k]), int(b[k]))
        assert su["pack_fused"] == su["pack_fused_fb_serial"] == su["pack_fused_fb_gc"] == 0, su
        for k in ("ops", "pack", "pack_scour", "pack_scour_nop", "pack_self_changed", "pack_sib_changed", "pack_one_row",
                  "pack_two_rows", "pack_serial", "pack_gc", "pack_cascade", "pack_grows", "pack_m_sum", "pack_kk_sum",
                  "scour", "scour_nop", "scour_serial", "move_slots", "lru_push"):
            assert sf[k] == su[k], (k, sf[k], su[k])
        # a pack is fused or handed back, and a pack handed back is one the sibling loop shapes as such
        assert sf["pack_fused"] + sf["pack_fused_fb_serial"] + sf["pack_fused_fb_gc"] <= sf["pack"], sf
        assert sf["pack_fused_fb_serial"] == sf["pack_serial"], sf
        return sf

    yield run
    regcpu._lib = base


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


def test_c4_longest_document_prefix(both):
    """The first 200 000 ops of C4's longest document: every pack is fused, none is handed back."""
    ops, pay = regcpu.generated(2, 111877, 200_000, n_clients=8, seed=1000)
    st = both(lambda: [regcpu.compare(ops, pay)])
    assert st["ops"] == 200_000 and st["pack_fused"] > 10_000, st
    assert st["pack_fused"] == st["pack"] and st["pack_fused_fb_serial"] == 0 and st["pack_fused_fb_gc"] == 0, st
    assert st["pack_two_rows"] > 0 and st["pack_cascade"] > 0 and st["pack_grows"] > 0 and st["pack_self_changed"] > 0, st


def test_kind5_fixed_rows_and_paged_pool(both):
    """Kind 5 (zamboni after nearly every op), 20 000 ops: the fixed rows fuse every pack, the paged pool
    (pool_rows=32) keeps the sibling loop -- as many packs again, none of them fused."""
    ops, pay = regcpu.generated(5, 29, 20_000, n_clients=8, seed=1000)
    st = both(lambda: [regcpu.compare(ops, pay)])
    assert st["pack_fused"] == st["pack"] > 1000 and st["pack_two_rows"] > 0 and st["pack_cascade"] > 0, st
    sp = both(lambda: [regcpu.compare(ops, pay, pool_rows=32)])
    assert sp["pack"] == st["pack"] and sp["pack_fused"] == 0, sp


@pytest.mark.parametrize("clients", [8, 31])
def test_kind3_joins_by_properties(both, clients):
    """Kind 3: match_props decides the joins whose property ids differ."""
    ops, pay = regcpu.generated(3, 7 + clients, 5000, n_clients=clients, seed=1000)
    st = both(lambda: [regcpu.compare_props(ops, pay)])
    assert st["pack_fused"] == st["pack"] > 0 and st["pack_sib_changed"] > 0, st


def test_wide_33_writers(both):
    """33 writers on the PROPS + WIDE engine (the second removers word travels through the gather)."""
    ops, pay = regcpu.generated(2, 3, 1200, n_clients=33, seed=1000)
    st = both(lambda: [regcpu.compare_props(ops, pay, wide=True)])
    assert st["pack_fused"] == st["pack"] > 0 and st["rem"] > 0, st


def test_serial_walk_hands_the_pack_back(both):
    """Inserts of 1..600 characters: packs with a joining slot longer than GRANULARITY go back to the
    sibling loop before any side effect, beside fused packs in the same document."""
    ops, pay, names = _builder_ops(long_insert_log())
    st = both(lambda: [regcpu.compare(ops, pay, names=names)])
    assert st["pack_fused_fb_serial"] > 0 and st["pack_fused"] > 0, st
    assert st["pack_fused"] + st["pack_fused_fb_serial"] == st["pack"], st


def test_arena_gc_hands_the_pack_back(both):
    """Kind 5 in an arena so small that packs find no room for their fresh chunks: they go back to the
    sibling loop, whose scour runs arena_gc; the document still replays (status 0, equal to the oracle)."""
    ops, pay = regcpu.generated(5, 0, 2000, n_clients=8, seed=1000)
    res = []

    def go():
        res.append(regcpu.compare(ops, pay, arena_cap=GC_ARENA_CAP))
        return res[-1:]

    st = both(go)
    assert all(int(r["status"]) == 0 and int(r["n_gc"]) > 0 for r in res), res
    assert st["pack_fused_fb_gc"] > 0 and st["pack_gc"] >= st["pack_fused_fb_gc"] and st["pack_fused"] > 0, st


def test_popped_block_joins_across_its_dropped_tombstone(both):
    """The hand-written log: text, a tombstone that drops, text in the popped block."""
    ops, pay, names = _builder_ops(tombstone_log())
    assert len(ops) < 40
    st = both(lambda: [regcpu.compare(ops, pay, names=names)])
    assert st["pack_self_changed"] > 0 and st["pack_fused"] == st["pack"] > 0, st


@pytest.mark.parametrize("kind,n_ops,clients,gid,seed", SOLO_DOCS)
def test_gpu_k_solo_documents_reach_their_shapes(both, kind, n_ops, clients, gid, seed):
    """The generated documents tests/test_gpu_pack_gather.py replays on k_solo."""
    ops, pay = regcpu.generated(kind, gid, n_ops, n_clients=clients, seed=seed)
    if kind == 3 or clients > 32:
        st = both(lambda: [regcpu.compare_props(ops, pay, wide=True)])
    else:
        st = both(lambda: [regcpu.compare(ops, pay)])
    assert st["pack_fused"] == st["pack"] > 0 and st["pack_sib_changed"] > 0, st
    if kind == 2 and clients == 8:
        assert st["pack_two_rows"] > 0 and st["pack_cascade"] > 0, st


@pytest.mark.parametrize("gid", [0, 1])
@pytest.mark.parametrize("kind,n_ops", [(2, 3000), (3, 2000), (5, 2000)])
def test_gpu_k_rows_documents_reach_their_shapes(both, kind, n_ops, gid):
    """The first two of the 48 documents the GPU file replays on k_rows, on the fixed rows (fused) and on
    the paged pool (the sibling loop): the same packs either way."""
    ops, pay = regcpu.generated(kind, gid, n_ops, n_clients=8, seed=1000)
    cmp = (lambda pool: regcpu.compare_props(ops, pay, pool_rows=pool)) if kind == 3 else \
          (lambda pool: regcpu.compare(ops, pay, pool_rows=pool or None))
    st = both(lambda: [cmp(0)])
    sp = both(lambda: [cmp(32)])
    assert st["pack_fused"] == st["pack"] == sp["pack"] > 0 and sp["pack_fused"] == 0, (st, sp)
    if kind == 2:
        assert st["pack_two_rows"] > 0 and st["pack_cascade"] > 0, st
