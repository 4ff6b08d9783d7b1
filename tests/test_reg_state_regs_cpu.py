"""The places of the row engine that round 13 looked at (reg_engine.hpp): CPU build,
bit-exact against the oracle on status, segment table and text, on documents built to reach every one of
them -- and the engine's event counters (MTE_CPU_STATS; tools/rg_stats.py names them) show that each is
reached. The lean engine's heap writes (kHeapInPlace) and packs' divisions (kMulDiv) are the code that
changed; the resolves, the block splits, room() and everything on the PROPS + WIDE engine are coverage of
code that stayed as it was:
  * a resolve that hits in its first row buffer and one that hits in its second, in documents of three or
    more rows (hit_first / hit_second count only those);
  * a block split of block k with k & 7 == 7, whose new block starts the next row (split_next_row);
  * heap entries written past position 63 (register 1: heap_reg1) and past 127 (registers 2..7: heap_reg2),
    and pops of a heap past 127 entries, which take the serial sift (sift_serial);
  * packs with every kk from 1 to 7 (pack_kk1 .. pack_kk7) and with T % kk != 0 (pack_rem);
  * cascades into pack_internal;
  * an op refused by room(): the document hands over between two ops (room_refused).
The pack's division by multiplier is checked against / and % for every T in 0..64 and kk in 1..7 by the
stand-alone program of tests/native/state_regs_main.cpp."""
import ctypes
import importlib.util
import os
import subprocess

import pytest

from tests import regcpu
from tests.state_regs_docs import FULL, HANDOFF, HANDOFF_AT, LEAN, W33

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NATIVE = os.path.join(_ROOT, "tests", "native")


def _names():
    spec = importlib.util.spec_from_file_location("rg_stats", os.path.join(_ROOT, "tools", "rg_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.NAMES


@pytest.fixture(scope="module")
def stats():
    """Routes tests.regcpu through the statistics build; stats(fn) runs fn and returns the event counts of
    the replays it made."""
    base = regcpu.lib()
    subprocess.run(["make", "-s", "-C", _NATIVE, "stats"], check=True)
    L = ctypes.CDLL(os.path.join(_NATIVE, "_build", "libregcpu_stats.so"))
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
        return {k: int(out[i]) for i, k in enumerate(names)}

    yield run
    regcpu._lib = base


def _gen(doc):
    kind, gid, n_ops, clients, seed = doc
    return regcpu.generated(kind, gid, n_ops, n_clients=clients, seed=seed)


def test_lean_document_reaches_the_restated_places(stats):
    ops, pay = _gen(LEAN)
    res = []
    st = stats(lambda: res.append(regcpu.compare(ops, pay)))
    assert int(res[0]["status"]) == 0 and int(res[0]["max_lb"]) > 16, res[0]  # three rows and more
    assert st["hit_first"] > 0 and st["hit_second"] > 0, st
    assert st["split_next_row"] > 0, st
    assert st["heap_reg1"] > 0, st  # the heap passed 64 entries
    for kk in range(1, 8):
        assert st["pack_kk%d" % kk] > 0, (kk, st)
    assert st["pack_rem"] > 0 and st["pack_internal"] > 0 and st["pack_cascade"] > 0, st
    assert st["room_refused"] == 0


def test_full_document_on_the_wide_engine(stats):
    ops, pay = _gen(FULL)
    st = stats(lambda: regcpu.compare_props(ops, pay, wide=True))
    assert st["hit_first"] > 0 and st["hit_second"] > 0 and st["split_next_row"] > 0, st
    assert st["pack"] > 0 and st["pack_rem"] > 0 and st["pack_internal"] > 0, st


def test_33_writers_heap_past_127(stats):
    ops, pay = _gen(W33)
    st = stats(lambda: regcpu.compare_props(ops, pay, wide=True))
    assert st["heap_reg1"] > 0 and st["heap_reg2"] > 0, st
    assert st["sift_serial"] > 0 and st["sift_serial"] == st["pop_big"], st


def test_room_refuses_an_op_and_the_document_hands_over(stats):
    """room() refuses op HANDOFF_AT: the engine stops there untouched by that op (the ops before it,
    replayed alone, are the oracle's); on the way the lean engine's heap passes 127 entries."""
    ops, pay = _gen(HANDOFF)
    out = []
    st = stats(lambda: out.append(regcpu.replay(ops, pay)))
    at, res = out[0][0], out[0][1]
    assert int(res["status"]) == regcpu.REG_HANDOFF and at == HANDOFF_AT, (at, res)
    assert st["room_refused"] == 1 and st["ops"] == HANDOFF_AT + 1, st
    assert st["heap_reg2"] > 0 and st["sift_serial"] > 0, st
    prefix = regcpu.compare(ops[:at], pay)
    assert int(prefix["status"]) == 0, prefix


def test_pack_division_by_multiplier_is_exact():
    subprocess.run(["make", "-s", "-C", _NATIVE, "-f", "state_regs.mk", "_build/state_regs_main"], check=True)
    r = subprocess.run([os.path.join(_NATIVE, "_build", "state_regs_main"), "--div"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "div ok %d" % (65 * 7), (r.stdout, r.stderr[-2000:])
