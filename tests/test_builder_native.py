"""The builder stands alone: fluidframework_amd/csrc/builder.cpp compiled with tests/native/builder_main.cpp
as a host program under AddressSanitizer and UBSan, linked without the HIP runtime and without
libmte.so, must build the same batch as mte.Builder (which loads libmte.so) from the same inputs."""
import ctypes
import os
import subprocess

from fluidframework_amd import mte
from tests.oplog import dumps
from tests.test_builder_cpu import random_log
from tests.test_oracle_specs import hello_world_log
from tests.test_summary_load import OBS, fixture, oracle_catchup, rebuild_edits

_NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
_PROG = os.path.join(_NATIVE, "_build", "builder_main")


def fnv1a(data):
    h = 0xCBF29CE484222325
    for x in data:
        h = ((h ^ x) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def batch_lines(b):
    """builder_main's output for batch b: name, element count and FNV-1a-64 of every array."""
    n = b.n_docs
    nkv = 0
    ps = (ctypes.c_uint32 * (2 * b.n_propsets)).from_address(b.propsets)
    for i in range(b.n_propsets):
        nkv = max(nkv, ps[2 * i] + ps[2 * i + 1])
    names = b.doc_client_offsets[n]

    def addr(p):
        return p if isinstance(p, int) else ctypes.cast(p, ctypes.c_void_p).value

    arrays = [("doc_op_offsets", b.doc_op_offsets, n + 1, 8), ("ops", b.ops, b.doc_op_offsets[n], 32),
              ("doc_payload_offsets", b.doc_payload_offsets, n + 1, 8), ("payload", b.payload, b.doc_payload_offsets[n], 2),
              ("propsets", b.propsets, b.n_propsets, 8), ("prop_keys", b.prop_keys, nkv, 4), ("prop_vals", b.prop_vals, nkv, 4),
              ("key_offsets", b.key_offsets, b.n_keys + 1, 8), ("key_text", b.key_text, b.key_offsets[b.n_keys], 1),
              ("val_offsets", b.val_offsets, b.n_vals + 1, 8), ("val_text", b.val_text, b.val_offsets[b.n_vals], 1),
              ("doc_client_offsets", b.doc_client_offsets, n + 1, 4),
              ("client_name_offsets", b.client_name_offsets, names + 1, 8),
              ("client_names", b.client_names, b.client_name_offsets[names], 1)]
    out = []
    for name, p, count, elem in arrays:
        data = ctypes.string_at(addr(p), count * elem) if count else b""
        out.append("%s %d %016x" % (name, count, fnv1a(data)))
    return out


def test_builder_standalone_matches_library(tmp_path):
    subprocess.run(["make", "-s", "-C", _NATIVE, "_build/builder_main"], check=True)
    # the link has neither the HIP runtime nor libmte.so
    needed = subprocess.run(["ldd", _PROG], check=True, capture_output=True, text=True).stdout
    assert "amdhip" not in needed and "libmte" not in needed, needed

    summary = fixture("headerAndBody")
    suffix = rebuild_edits(oracle_catchup(summary, None).length())
    opened = random_log(2)
    cut = len(opened) // 2
    texts = {"hello.json": dumps(hello_world_log()), "random1.json": dumps(random_log(1)), "summary.json": summary,
             "suffix.json": dumps(suffix), "open_a.json": dumps(opened[:cut]), "open_b.json": dumps(opened[cut:])}
    path = {}
    for name, text in texts.items():
        path[name] = str(tmp_path / name)
        with open(path[name], "w", encoding="utf-8") as f:
            f.write(text)

    b = mte.Builder()
    b.add_doc(texts["hello.json"], observer="obs")
    b.add_doc(texts["random1.json"])
    b.add_doc_from_summary(summary, texts["suffix.json"], observer=OBS)
    d = b.open_doc()
    b.append(d, texts["open_a.json"])
    b.append(d, texts["open_b.json"])
    expected = batch_lines(b.batch())  # the only mte_builder_batch after the last append

    r = subprocess.run([_PROG, "doc", "obs", path["hello.json"], "doc", "__observer__", path["random1.json"],
                        "summary", OBS, path["summary.json"], path["suffix.json"],
                        "open", "__observer__", path["open_a.json"], path["open_b.json"]],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert r.stderr == "", r.stderr[-2000:]  # no sanitizer report
    assert r.stdout.splitlines() == expected
