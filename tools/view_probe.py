"""Time of the view queries (mte_views) against the route that existed before them, on the GPU.

After one replay of the C2 shape (4 096 documents x 10^4 generated ops) it times one mte_views call with
1, 64 and 4 096 random LOCATE queries per document (random writers and reference sequence numbers inside
each document's window), and with 64 TEXT queries of at most 256 units per document. The comparison is the
route the same library offers without them: the first mte_segments_json call of a replay (the whole
output pool copied to the host) plus a host walk of the document's rows per query (bisect over the
cumulative lengths, the view already prepared).

Each figure is a host clock around a call that ends in a device synchronise (mte_views returns after its
results are copied out). The first call of a shape allocates the call's device buffers and is reported
apart ("first_ms"); then `--repeats` calls, reported as median, min and max.

  python tools/view_probe.py --out profiles/r11/views.json"""
import argparse
import bisect
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


def main():
    from fluidframework_amd import mte

    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--ops", type=int, default=10000)
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()

    e = mte.Engine(0)
    e.generate(2, a.docs, a.ops, n_clients=a.clients, seed=1)
    st = e.replay()
    assert st["failed_docs"] == 0, st
    rng = np.random.default_rng(11)
    # each document's window and observer length, through the queries themselves
    win = np.array([[e.doc_result(d)[k] for k in ("min_seq", "cur_seq", "n_segs")] for d in range(a.docs)], dtype=np.int64)
    q = np.zeros(a.docs, dtype=mte.VIEW_Q_DTYPE)
    q["doc"] = np.arange(a.docs)
    q["kind"] = mte.MTE_VQ_LENGTH
    t0 = time.perf_counter()
    lens, _ = e.views(q)
    first_length_ms = (time.perf_counter() - t0) * 1e3
    L = lens["length"].astype(np.int64)

    def queries(per_doc, kind, span=0):
        n = a.docs * per_doc
        q = np.zeros(n, dtype=mte.VIEW_Q_DTYPE)
        d = np.repeat(np.arange(a.docs), per_doc)
        q["doc"] = d
        q["kind"] = kind
        q["client"] = rng.integers(1, a.clients + 1, n)
        q["ref_seq"] = rng.integers(win[d, 0], win[d, 1] + 1)
        q["pos1"] = rng.integers(0, np.maximum(L[d], 1))
        q["pos2"] = q["pos1"] + (rng.integers(0, span + 1, n) if span else 0)
        return q[rng.permutation(n)]

    out = {"workload": f"C2 shape: {a.docs} documents x {a.ops} generated ops, {a.clients} writers; one replay",
           "unit": "host clock around one mte_views call (plan, upload, kernels, download), ms",
           "replay_kernel_ms": round(st["kernel_ms"], 3), "rows": int(win[:, 2].sum()),
           "length_query_per_document_first_ms": round(first_length_ms, 3), "views": {}}
    for name, per_doc, kind, span in (("locate_1_per_doc", 1, mte.MTE_VQ_LOCATE, 0), ("locate_64_per_doc", 64, mte.MTE_VQ_LOCATE, 0),
                                      ("locate_4096_per_doc", 4096, mte.MTE_VQ_LOCATE, 0),
                                      ("text_64_per_doc_le_256_units", 64, mte.MTE_VQ_TEXT, 256)):
        qs = queries(per_doc, kind, span)
        res = np.zeros(len(qs), dtype=mte.VIEW_R_DTYPE)
        times, units = [], 0
        for rep in range(a.repeats + 1):
            t0 = time.perf_counter()
            res, txt = e.views(qs)
            times.append((time.perf_counter() - t0) * 1e3)
            units = len(txt)
        assert e.get_info("downloaded") == 0
        r = {"queries": len(qs), "first_ms": round(times[0], 3), **spread(times[1:]),
             "status_counts": {int(k): int(v) for k, v in zip(*np.unique(res["status"], return_counts=True))}}
        r["us_per_query"] = round(r["median_ms"] * 1e3 / len(qs), 4)
        if kind == mte.MTE_VQ_TEXT:
            r["text_units"] = units
        out["views"][name] = r
        print(name, r, flush=True)

    # the route without them: the whole-pool download (first segment-table read), then a host walk per query
    t0 = time.perf_counter()
    rows0 = json.loads(e.segments_json(0))
    download_ms = (time.perf_counter() - t0) * 1e3
    assert e.get_info("downloaded") == 1
    t0 = time.perf_counter()
    tables = [json.loads(e.segments_json(d)) for d in range(min(a.docs, 64))]
    table_ms = (time.perf_counter() - t0) * 1e3 / len(tables)
    ends, at = [], 0
    for r in rows0:
        at += 0 if "removedSeq" in r else r["len"]
        ends.append(at)
    t0 = time.perf_counter()
    for p in rng.integers(0, max(at, 1), 10000):
        bisect.bisect_right(ends, int(p))
    walk_us = (time.perf_counter() - t0) * 1e6 / 10000
    out["download_route"] = {"first_segments_call_ms": round(download_ms, 3),
                             "segment_table_per_document_ms": round(table_ms, 3),
                             "host_locate_us_per_query_prepared_view": round(walk_us, 3),
                             "note": "first_segments_call_ms is dominated by the copy of the whole output pool; a view "
                                     "other than the observer's also has to be prepared per (client, ref_seq) on the host"}
    print("download route", out["download_route"], flush=True)
    e.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
