"""The fused pack (reg_engine.hpp pack_fused) under ASan and UBSan: the statistics build of the CPU row
engine as a stand-alone host program (tests/native/pack_gather_main.cpp) replays three documents of
tests/test_reg_pack_gather_cpu.py in one run -- lean with siblings in two rows, PROPS + WIDE, and the
long inserts whose packs go back to the sibling loop for the serial walk -- with no sanitizer report, rows
and text equal to the oracle's, and the counters showing that the fused path and its fallback ran. A
stand-alone program only: no HIP in its link, no sanitizer loaded into Python."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from fluidframework_amd import mte
from oracle import _op_dtype
from tests import regcpu
from tests.oplog import dumps
from tests.pack_gather_docs import long_insert_log

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NATIVE = os.path.join(_ROOT, "tests", "native")
_PROG = os.path.join(_NATIVE, "_build", "pack_gather_main")
MAP_WORDS = 16


def _stat_names():
    spec = importlib.util.spec_from_file_location("rg_stats", os.path.join(_ROOT, "tools", "rg_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.NAMES


def _write(path, ops, pay, kind, gp=None):
    n = len(ops)
    seg_cap, arena_cap, map_cap = 3 * n + 8, 6 * len(pay) + 4096, 2 * n + 64
    hdr = np.array([n, len(pay), seg_cap, arena_cap, kind, 0, gp.n_propsets if gp else 0, len(gp.prop_keys) if gp else 0,
                    len(gp.VALS) if gp else 0, MAP_WORDS if gp else 0, map_cap, 0], dtype=np.uint64)
    with open(path, "wb") as f:
        f.write(hdr.tobytes() + ops.tobytes() + np.concatenate([pay, np.zeros(1, np.uint16)]).tobytes())
        if gp:
            f.write(gp.propsets.tobytes() + gp.prop_keys.tobytes() + gp.prop_vals.tobytes() + gp.val_flags.tobytes())


def _read(path, pay, gp):
    raw = open(path, "rb").read()
    res = np.frombuffer(raw, dtype=regcpu.DOCRES, count=1)[0]
    k, o = int(res["n_segs"]), regcpu.DOCRES.itemsize
    vis = np.frombuffer(raw, np.uint32, 4 * k, o).reshape(k, 4)
    aux = np.frombuffer(raw, np.uint32, 4 * k, o + 16 * k).reshape(k, 4)
    ovl = np.frombuffer(raw, np.uint64, k, o + 32 * k)
    text = np.frombuffer(raw, np.uint16, len(pay) + 16, o + 40 * k)
    mw = MAP_WORDS if gp else 0
    maps = np.frombuffer(raw, np.uint32, k * mw, o + 40 * k + 2 * (len(pay) + 16)).reshape(k, mw) if mw else None
    return res, (vis, aux, ovl), text, maps


def _gen_names(ops):
    return ["__observer__"] + [f"w{i}" for i in range(1, max(int(ops["client"].max()), 1) + 1)]


def test_three_documents_under_sanitizers(tmp_path):
    subprocess.run(["make", "-s", "-C", _NATIVE, "-f", "pack_gather.mk", "_build/pack_gather_main"], check=True)
    needed = subprocess.run(["ldd", _PROG], check=True, capture_output=True, text=True).stdout
    assert "amdhip64" not in needed and "libmte" not in needed, needed
    gp = regcpu.GenProps()
    docs = []
    ops, pay = regcpu.generated(2, 1, 3000, n_clients=8, seed=17)
    docs.append((ops, pay, _gen_names(ops), 0, None))
    ops, pay = regcpu.generated(3, 7, 2000, n_clients=8, seed=1000)
    docs.append((ops, pay, _gen_names(ops), 3, gp))
    b = mte.Builder()
    b.add_doc(dumps(long_insert_log()))
    batch = b.batch()
    n_pay = batch.doc_payload_offsets[1]
    cno = batch.client_name_offsets
    docs.append((mte.batch_ops(batch).copy(), np.ctypeslib.as_array(batch.payload, shape=(max(n_pay, 1),))[:n_pay].copy(),
                 [ctypes.string_at(batch.client_names + cno[i], cno[i + 1] - cno[i]).decode()
                  for i in range(batch.doc_client_offsets[1])], 0, None))
    args = []
    for i, (ops, pay, _, kind, g) in enumerate(docs):
        docs[i] = (np.ascontiguousarray(ops, dtype=_op_dtype()), np.ascontiguousarray(pay, dtype=np.uint16)) + docs[i][2:]
        _write(tmp_path / f"in{i}.bin", docs[i][0], docs[i][1], kind, g)
        args += [str(tmp_path / f"in{i}.bin"), str(tmp_path / f"out{i}.bin")]
    r = subprocess.run([_PROG] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    names = _stat_names()
    lines = [x.split()[1:] for x in r.stdout.splitlines() if x.startswith("stats ")]
    assert len(lines) == 3 and all(len(x) == len(names) for x in lines), "tools/rg_stats.py NAMES and RgStat differ"
    sts = [dict(zip(names, (int(v) for v in x))) for x in lines]
    for i, (ops, pay, cl, kind, g) in enumerate(docs):
        res, rows, text, maps = _read(tmp_path / f"out{i}.bin", pay, g)
        o = regcpu.OneDocBatch(ops, pay, cl, gp=g).oracle()
        assert int(res["status"]) == o.status()[0] == 0
        props = (lambda j: g.render(maps[j])) if g else None
        assert regcpu.rows_json(rows, text, cl, props=props) == o.segments_json()
        assert regcpu.engine_text(rows, text) == o.text()
    lean, wide, serial = sts
    assert lean["pack_fused"] == lean["pack"] > 0 and lean["pack_two_rows"] > 0 and lean["pack_cascade"] > 0, lean
    assert wide["pack_fused"] == wide["pack"] > 0 and wide["pack_sib_changed"] > 0, wide
    assert serial["pack_fused_fb_serial"] > 0 and serial["pack_fused"] > 0, serial
