"""Time of the marker queries (mte_markers) against the route that existed before them, on the GPU.

The workload is the C2 shape (4 096 documents x 10^4 generated ops) with tile markers: the generated batch
is exported, every second one-unit text insert becomes a Tile marker carrying referenceTileLabels ["EOP"]
(a marker is as long as the text it replaces, so every later position stays valid), and the batch is loaded
and replayed once. Some of the patched logs no longer replay (an insert fails, in the oracle too): their
queries answer MTE_MARK_DOC_FAILED, and the output records how many ("failed_docs"). Then it times one mte_markers call with 1 and with 64 TILE queries per document (random
positions, both directions) and with the PARAGRAPHS of every document. The comparison is the route the
same library offers without them: the first mte_segments_json call of a replay (the whole output pool
copied to the host), then per document its segment table and a host scan that parses each marker's
property JSON.

Each figure is a host clock around a call that ends in a device synchronise (mte_markers returns after its
results are copied out). The first call of a shape allocates the call's device buffers (the very first one
also builds the label's bitmap and derives the annotate flags) and is reported apart ("first_ms"); then
`--repeats` calls, reported as median, min and max. Not measured here: the host plan's share of a call, and
the kernels alone.

  python tools/marker_probe.py --out profiles/r15/markers.json"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "repeats": len(ms)}


def with_tiles(mte, b):
    """The exported batch b with tile markers: (patched mte_batch, number of markers). The arrays it points to
    are kept alive on the returned object."""
    ops = mte.batch_ops(b).copy()
    one = np.flatnonzero((ops["type"] == 0) & (ops["b"] == 1))[::2]
    assert len(one), "the generated batch has no one-unit insert"

    def arr(ptr, n, dt):
        return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt).copy() if n else np.zeros(0, dt)

    n_ps, n_keys, n_vals = b.n_propsets, b.n_keys, b.n_vals
    sets = np.frombuffer((ctypes.c_char * (n_ps * 8)).from_address(b.propsets), dtype="<u4").reshape(n_ps, 2).copy()
    n_kv = int((sets[:, 0] + sets[:, 1]).max()) if n_ps else 0
    keys, vals = arr(b.prop_keys, n_kv, np.uint32), arr(b.prop_vals, n_kv, np.uint32)
    key_off, val_off = arr(b.key_offsets, n_keys + 1, np.uint64), arr(b.val_offsets, n_vals + 1, np.uint64)
    key_text = (ctypes.string_at(b.key_text, int(key_off[-1])) if key_off[-1] else b"") + b'"referenceTileLabels"'
    val_text = ctypes.string_at(b.val_text, int(val_off[-1])) + b'["EOP"]'
    keep = {"ops": ops, "sets": np.vstack([sets, [[n_kv, 1]]]).astype("<u4"), "keys": np.append(keys, n_keys).astype(np.uint32),
            "vals": np.append(vals, n_vals).astype(np.uint32), "key_off": np.append(key_off, len(key_text)).astype(np.uint64),
            "val_off": np.append(val_off, len(val_text)).astype(np.uint64), "key_text": ctypes.create_string_buffer(key_text),
            "val_text": ctypes.create_string_buffer(val_text)}
    ops["type"][one] = 3  # MTE_OP_INSERT_MARKER: b = refType
    ops["b"][one] = 1     # ReferenceType.Tile
    ops["props"][one] = n_ps
    p = mte.mte_batch()
    ctypes.memmove(ctypes.byref(p), ctypes.byref(b), ctypes.sizeof(p))
    p.ops = keep["ops"].ctypes.data
    p.n_propsets, p.propsets = n_ps + 1, keep["sets"].ctypes.data
    p.prop_keys = keep["keys"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    p.prop_vals = keep["vals"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    p.n_keys, p.key_offsets = n_keys + 1, keep["key_off"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    p.key_text = ctypes.addressof(keep["key_text"])
    p.n_vals, p.val_offsets = n_vals + 1, keep["val_off"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    p.val_text = ctypes.addressof(keep["val_text"])
    p._keep = (keep, b)
    return p, len(one)


def host_scan(rows, label="EOP"):
    """What a caller does today per document: every marker's property JSON parsed, the tiles' positions."""
    out, at = [], 0
    for r in rows:
        n = 0 if "removedSeq" in r else r["len"]
        if n and r["kind"] == "M" and r["refType"] & 1 and r["props"]:
            v = json.loads(r["props"]).get("referenceTileLabels")
            if isinstance(v, (list, str)) and label in v:
                out.append(at)
        at += n
    return out


def main():
    from fluidframework_amd import mte

    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--ops", type=int, default=10000)
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()

    g = mte.Engine(0)
    g.generate(2, a.docs, a.ops, n_clients=a.clients, seed=1)
    batch, n_markers = with_tiles(mte, g.export_batch())
    e = mte.Engine(0)
    e.load(batch)
    st = e.replay()
    # documents whose replay fails answer MTE_MARK_DOC_FAILED without reaching the device; they are counted
    # below, and the oracle's verdict on the first of them is recorded beside the engine's
    failed = [d for d in range(a.docs) if e.status(d)[0]] if st["failed_docs"] else []
    oracle_says = None
    if failed:
        from oracle import replay_batch

        oracle_says = int(replay_batch(ctypes.addressof(batch), failed[0], failed[0] + 1, threads=1)[2][0])
    g.close()
    rng = np.random.default_rng(11)
    q = np.zeros(a.docs, dtype=mte.VIEW_Q_DTYPE)
    q["doc"] = np.arange(a.docs)
    q["kind"] = mte.MTE_VQ_LENGTH
    L = e.views(q)[0]["length"].astype(np.int64)
    rows = sum(e.doc_result(d)["n_segs"] for d in range(a.docs))

    def tiles(per_doc):
        n = a.docs * per_doc
        q = np.zeros(n, dtype=mte.MARK_Q_DTYPE)
        d = np.repeat(np.arange(a.docs), per_doc)
        q["doc"] = d
        q["kind"] = rng.integers(0, 2, n)  # TILE_BEFORE / TILE_AFTER
        q["pos1"] = rng.integers(0, np.maximum(L[d], 1))
        return q[rng.permutation(n)]

    para = np.zeros(a.docs, dtype=mte.MARK_Q_DTYPE)
    para["doc"] = np.arange(a.docs)
    para["kind"] = mte.MTE_MQ_PARAGRAPHS
    para["pos2"] = mte.MTE_MARK_TO_END
    out = {"workload": f"C2 shape: {a.docs} documents x {a.ops} generated ops, {a.clients} writers, {n_markers} of the "
                       f"one-unit inserts turned into Tile markers; one replay",
           "unit": "host clock around one mte_markers call (plan, upload, kernels, download), ms",
           "not_measured": "the host plan's share of a call; the kernels alone",
           "replay_kernel_ms": round(st["kernel_ms"], 3), "rows": int(rows), "failed_docs": len(failed), "markers": {}}
    if failed:
        out["first_failed_doc"] = {"doc": failed[0], "engine_status": e.status(failed[0])[0], "oracle_status": oracle_says}
    for name, qs in (("tile_1_per_doc", tiles(1)), ("tile_64_per_doc", tiles(64)), ("paragraphs_every_doc", para)):
        times = []
        for rep in range(a.repeats + 1):
            t0 = time.perf_counter()
            res, pieces, text = e.markers(qs, ["EOP"])
            times.append((time.perf_counter() - t0) * 1e3)
        assert e.get_info("downloaded") == 0
        r = {"queries": len(qs), "first_ms": round(times[0], 3), **spread(times[1:]),
             "status_counts": {int(k): int(v) for k, v in zip(*np.unique(res["status"], return_counts=True))}}
        r["us_per_query"] = round(r["median_ms"] * 1e3 / len(qs), 4)
        if name.startswith("paragraphs"):
            r["pieces"], r["text_units"] = len(pieces), len(text)
        out["markers"][name] = r
        print(name, r, flush=True)

    # the route without them: the whole-pool download (first segment-table read), then a table and a scan per document
    t0 = time.perf_counter()
    e.segments_json(0)
    download_ms = (time.perf_counter() - t0) * 1e3
    assert e.get_info("downloaded") == 1
    good = [d for d in range(a.docs) if d not in set(failed)][:64]
    n = len(good)
    t0 = time.perf_counter()
    found = sum(len(host_scan(json.loads(e.segments_json(d)))) for d in good)
    scan_ms = (time.perf_counter() - t0) * 1e3 / n
    out["download_route"] = {"first_segments_call_ms": round(download_ms, 3),
                             "segment_table_and_scan_per_document_ms": round(scan_ms, 3),
                             "all_documents_ms_extrapolated": round(download_ms + scan_ms * a.docs, 1),
                             "tiles_found_in_the_scanned_documents": found,
                             "note": "first_segments_call_ms is dominated by the copy of the whole output pool; the "
                                     f"per-document figure is the mean over the first {n} replayed documents"}
    print("download route", out["download_route"], flush=True)
    e.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
