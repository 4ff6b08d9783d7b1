"""The statistics build of the CPU row engine as a stand-alone host program under ASan and UBSan
(tests/native/state_regs_main.cpp): the documents of tests/test_reg_state_regs_cpu.py replayed through it
-- on the lean engine heap entries written by lane compare in registers 0..7 and the packs' division by a
multiplier with every kk; the serial sift; on the PROPS + WIDE engine the code as it was -- with no
sanitizer report, rows and text equal to the oracle's, and the event counters showing that the replay met
those places. A stand-alone program only: no sanitizer is loaded into Python."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from oracle import _op_dtype
from tests import regcpu
from tests.state_regs_docs import FULL, HANDOFF, HANDOFF_AT, LEAN, W33

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NATIVE = os.path.join(_ROOT, "tests", "native")
_PROG = os.path.join(_NATIVE, "_build", "state_regs_main")


def _stat_names():
    spec = importlib.util.spec_from_file_location("rg_stats", os.path.join(_ROOT, "tools", "rg_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.NAMES


@pytest.fixture(scope="module")
def prog():
    subprocess.run(["make", "-s", "-C", _NATIVE, "-f", "state_regs.mk", "_build/state_regs_main"], check=True)
    needed = subprocess.run(["ldd", _PROG], check=True, capture_output=True, text=True).stdout
    assert "amdhip64" not in needed and "libmte" not in needed, needed
    return _PROG


def _replay(prog, tmp_path, ops, pay, kind, gp=None, map_words=16):
    ops = np.ascontiguousarray(ops, dtype=_op_dtype())
    pay = np.ascontiguousarray(pay, dtype=np.uint16)
    n = len(ops)
    seg_cap, arena_cap, map_cap = 3 * n + 8, 6 * len(pay) + 4096, 2 * n + 64
    n_kv = len(gp.prop_keys) if gp else 0
    hdr = np.array([n, len(pay), seg_cap, arena_cap, kind, 0, gp.n_propsets if gp else 0, n_kv,
                    len(gp.VALS) if gp else 0, map_words if gp else 0, map_cap, 0], dtype=np.uint64)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(hdr.tobytes() + ops.tobytes() + np.concatenate([pay, np.zeros(1, np.uint16)]).tobytes())
        if gp:
            f.write(gp.propsets.tobytes() + gp.prop_keys.tobytes() + gp.prop_vals.tobytes() + gp.val_flags.tobytes())
    r = subprocess.run([prog, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    stop = int(r.stdout.split("stop=")[1].split()[0])
    line = [x for x in r.stdout.splitlines() if x.startswith("stats ")][0].split()[1:]
    names = _stat_names()
    assert len(line) == len(names), "tools/rg_stats.py NAMES and RgStat differ"
    st = dict(zip(names, (int(x) for x in line)))
    raw = dst.read_bytes()
    res = np.frombuffer(raw, dtype=regcpu.DOCRES, count=1)[0]
    k, o = int(res["n_segs"]), regcpu.DOCRES.itemsize
    vis = np.frombuffer(raw, np.uint32, 4 * k, o).reshape(k, 4)
    aux = np.frombuffer(raw, np.uint32, 4 * k, o + 16 * k).reshape(k, 4)
    ovl = np.frombuffer(raw, np.uint64, k, o + 32 * k)
    text = np.frombuffer(raw, np.uint16, len(pay) + 16, o + 40 * k)
    mw = map_words if gp else 0
    maps = np.frombuffer(raw, np.uint32, k * mw, o + 40 * k + 2 * (len(pay) + 16)).reshape(k, mw) if mw else None
    return stop, res, (vis, aux, ovl), text, maps, st


def _gen(doc):
    kind, gid, n_ops, clients, seed = doc
    return regcpu.generated(kind, gid, n_ops, n_clients=clients, seed=seed)


def _names(ops):
    return ["__observer__"] + [f"w{i}" for i in range(1, max(int(ops["client"].max()), 1) + 1)]


def test_lean_document_under_sanitizers(prog, tmp_path):
    ops, pay = _gen(LEAN)
    names = _names(ops)
    _, res, rows, text, _, st = _replay(prog, tmp_path, ops, pay, 0)
    o = regcpu.OneDocBatch(ops, pay, names).oracle()
    assert int(res["status"]) == o.status()[0] == 0 and int(res["max_lb"]) > 16
    assert regcpu.rows_json(rows, text, names) == o.segments_json()
    assert regcpu.engine_text(rows, text) == o.text()
    assert st["hit_first"] > 0 and st["hit_second"] > 0 and st["split_next_row"] > 0 and st["heap_reg1"] > 0, st
    assert all(st["pack_kk%d" % kk] > 0 for kk in range(1, 8)) and st["pack_rem"] > 0 and st["pack_internal"] > 0, st


@pytest.mark.parametrize("doc", [FULL, W33])
def test_wide_documents_under_sanitizers(prog, tmp_path, doc):
    """Properties and annotates on the PROPS + WIDE engine; 33 writers: a heap past 127 entries, the serial sift."""
    gp = regcpu.GenProps()
    ops, pay = _gen(doc)
    names = _names(ops)
    _, res, rows, text, maps, st = _replay(prog, tmp_path, ops, pay, 3, gp=gp)
    o = regcpu.OneDocBatch(ops, pay, names, gp=gp).oracle()
    assert int(res["status"]) == o.status()[0] == 0
    assert regcpu.rows_json(rows, text, names, props=lambda i: gp.render(maps[i])) == o.segments_json()
    assert regcpu.engine_text(rows, text) == o.text()
    assert st["pack"] > 0 and st["hit_second"] > 0, st
    if doc is W33:
        assert st["heap_reg2"] > 0 and st["sift_serial"] > 0, st


def test_handoff_document_under_sanitizers(prog, tmp_path):
    """The lean engine up to the op room() refuses: the heap's registers 2..7 and the serial sift on the way."""
    ops, pay = _gen(HANDOFF)
    stop, res, _, _, _, st = _replay(prog, tmp_path, ops, pay, 0)
    assert stop == HANDOFF_AT and int(res["status"]) == regcpu.REG_HANDOFF, (stop, res)
    assert st["room_refused"] == 1 and st["heap_reg2"] > 0 and st["sift_serial"] > 0, st
