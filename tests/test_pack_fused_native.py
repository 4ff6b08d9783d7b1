"""The statistics build of the CPU row engine as a stand-alone host program under ASan and UBSan
(tests/native/pack_fused_main.cpp): two documents of tests/test_reg_pack_fused_cpu.py replayed through it
-- packs with siblings in two rows, cascades into pack_internal, needsScour marks folded into the edit's
row write -- with no sanitizer report, rows and text equal to the oracle's, and the event counters
showing that the replay met those paths. A stand-alone program only: no sanitizer is loaded into Python."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from oracle import _op_dtype
from tests import regcpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NATIVE = os.path.join(_ROOT, "tests", "native")
_PROG = os.path.join(_NATIVE, "_build", "pack_fused_main")


def _stat_names():
    spec = importlib.util.spec_from_file_location("rg_stats", os.path.join(_ROOT, "tools", "rg_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.NAMES


@pytest.fixture(scope="module")
def prog():
    subprocess.run(["make", "-s", "-C", _NATIVE, "-f", "pack_fused.mk", "_build/pack_fused_main"], check=True)
    needed = subprocess.run(["ldd", _PROG], check=True, capture_output=True, text=True).stdout
    assert "amdhip64" not in needed and "libmte" not in needed, needed
    return _PROG


def _replay(prog, tmp_path, ops, pay, kind, pool=0, gp=None, map_words=16):
    ops = np.ascontiguousarray(ops, dtype=_op_dtype())
    pay = np.ascontiguousarray(pay, dtype=np.uint16)
    n = len(ops)
    seg_cap, arena_cap, map_cap = 3 * n + 8, 6 * len(pay) + 4096, 2 * n + 64
    n_kv = len(gp.prop_keys) if gp else 0
    hdr = np.array([n, len(pay), seg_cap, arena_cap, kind, pool, gp.n_propsets if gp else 0, n_kv,
                    len(gp.VALS) if gp else 0, map_words if gp else 0, map_cap, 0], dtype=np.uint64)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(hdr.tobytes() + ops.tobytes() + np.concatenate([pay, np.zeros(1, np.uint16)]).tobytes())
        if gp:
            f.write(gp.propsets.tobytes() + gp.prop_keys.tobytes() + gp.prop_vals.tobytes() + gp.val_flags.tobytes())
    r = subprocess.run([prog, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
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
    return res, (vis, aux, ovl), text, maps, st


def _names(ops):
    return ["__observer__"] + [f"w{i}" for i in range(1, max(int(ops["client"].max()), 1) + 1)]


@pytest.mark.parametrize("kind,pool", [(0, 0), (1, 32)])
def test_kind2_packs_under_sanitizers(prog, tmp_path, kind, pool):
    """5 000 ops of C4's longest document, fixed rows and the paged pool."""
    ops, pay = regcpu.generated(2, 111877, 5000, n_clients=8, seed=1000)
    names = _names(ops)
    res, rows, text, _, st = _replay(prog, tmp_path, ops, pay, kind, pool)
    o = regcpu.OneDocBatch(ops, pay, names).oracle()
    assert int(res["status"]) == o.status()[0] == 0 and int(res["max_lb"]) > 8
    assert regcpu.rows_json(rows, text, names) == o.segments_json()
    assert regcpu.engine_text(rows, text) == o.text()
    assert st["pack_two_rows"] > 0 and st["pack_cascade"] > 0 and st["pack_self_changed"] > 0, st
    if kind == 0:  # a whole row store: the marks ride on the edit's row write but for splitting inserts
        assert st["lru_folded"] > st["lru_rewrite"] > 0, st
    else:  # the paged pool keeps add_lru's own write
        assert st["lru_folded"] == 0 and st["lru_rewrite"] == st["lru_push"] > 0, st


def test_kind3_wide_packs_under_sanitizers(prog, tmp_path):
    """Kind 3 on the PROPS + WIDE engine: joins by match_props, annotates (their marks are not folded)."""
    gp = regcpu.GenProps()
    ops, pay = regcpu.generated(3, 7, 2000, n_clients=8, seed=1000)
    names = _names(ops)
    res, rows, text, maps, st = _replay(prog, tmp_path, ops, pay, 3, gp=gp)
    o = regcpu.OneDocBatch(ops, pay, names, gp=gp).oracle()
    assert int(res["status"]) == o.status()[0] == 0
    assert regcpu.rows_json(rows, text, names, props=lambda i: gp.render(maps[i])) == o.segments_json()
    assert regcpu.engine_text(rows, text) == o.text()
    assert st["pack"] > 0 and st["lru_folded"] > 0 and st["lru_rewrite"] > 0, st
