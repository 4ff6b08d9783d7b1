"""Time of the SharedMatrix reads (mte_matrix_cells) against the route that existed before them, on the GPU.

Two batches, each replayed once: the 4 200 x 4 200 handle-levels matrix of tests/matrix_edges.py alone, and
1 000 copies of its 27 x 2 recycling matrix. On each it times one mte_matrix_cells call with the full-grid
RECT of every matrix, with 4 096 and with 262 144 random CELL queries. The comparison is the only route the
library had: mte_snapshot_matrix per matrix (the C call alone: both vectors' SnapshotV1 trees, the handle
tables and the cells blob built on the host) and that call plus the Python decode the tests use (json.loads
and tests/test_matrix_spec.py grid(); on the 4 200 x 4 200 matrix the decode is timed on its first
`--grid-rows` rows and scaled, since 17.6 M Python getCells take minutes).

Each figure is a host clock around a call that ends in a device synchronise. The first mte_matrix_cells call
of a batch builds the cell tables and is reported apart ("first_ms"); then `--repeats` calls, reported as
median, min and max.

  python tools/matrix_probe.py --out profiles/r14/matrix_reads.json"""
import argparse
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


def timed(fn, repeats):
    times, res = [], None
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        res = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"first_ms": round(times[0], 3), **spread(times[1:])}, res


def probe(mte, name, logs, a, rng):
    from tests.test_matrix_spec import get_cell, grid, vector_handles

    e = mte.Engine(0)
    b = mte.Builder()
    pairs = [b.add_matrix_log(log, observer="obs") for log in logs]
    e.load(b.batch())
    st = e.replay()
    assert st["failed_docs"] == 0, st
    out = {"matrices": len(pairs), "replay_kernel_ms": round(st["kernel_ms"], 3)}
    shape_q = np.zeros(len(pairs), dtype=mte.CELL_Q_DTYPE)
    shape_q["rows_doc"], shape_q["cols_doc"] = [p[0] for p in pairs], [p[1] for p in pairs]
    t0 = time.perf_counter()
    shapes, _ = e.matrix_cells(shape_q)   # the batch's first call: builds every table
    out["first_call_shapes_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    out["tables_built"] = e.get_info("mx_tables_built")
    R, C = shapes["row_count"].astype(np.int64), shapes["col_count"].astype(np.int64)
    out["cells"] = int((R * C).sum())

    full = shape_q.copy()
    full["kind"], full["n_rows"], full["n_cols"] = mte.MTE_MQ_RECT, R, C
    r, (res, vals) = timed(lambda: e.matrix_cells(full), a.repeats)
    assert (res["status"] == mte.MTE_MX_OK).all() and len(vals) == out["cells"]
    r["ids"] = len(vals)
    r["stored"] = int((vals != mte.MTE_CELL_NONE).sum())
    out["full_grid_rect"] = r
    print(name, "full_grid_rect", r, flush=True)
    for n in (4096, 262144):
        m = rng.integers(0, len(pairs), n)
        q = np.zeros(n, dtype=mte.CELL_Q_DTYPE)
        q["rows_doc"], q["cols_doc"], q["kind"] = shape_q["rows_doc"][m], shape_q["cols_doc"][m], mte.MTE_MQ_CELL
        q["row"], q["col"] = rng.integers(0, R[m]), rng.integers(0, C[m])
        r, (res, _) = timed(lambda: e.matrix_cells(q), a.repeats)
        assert (res["status"] == mte.MTE_MX_OK).all()
        r["us_per_query"] = round(r["median_ms"] * 1e3 / n, 4)
        r["stored"] = int((res["value"] != mte.MTE_CELL_NONE).sum())
        out[f"cells_{n}"] = r
        print(name, f"cells_{n}", r, flush=True)
    assert e.get_info("downloaded") == 0 and e.get_info("mx_tables_built") == out["tables_built"]

    # the route without them: the summary of every matrix, then the decode
    def snapshots():
        return [e.snapshot_matrix(*p) for p in pairs]

    r, raws = timed(snapshots, min(a.repeats, 3))
    r["bytes"] = sum(len(x) for x in raws)
    out["snapshot_matrix_all"] = r
    print(name, "snapshot_matrix_all", r, flush=True)
    t0 = time.perf_counter()
    trees = [json.loads(x) for x in raws]
    parse_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    if out["cells"] <= 1 << 20:
        grids = [grid(t) for t in trees]
        decoded, scale = sum(len(g) * len(g[0]) for g in grids if g), 1.0
    else:   # a sample of rows, scaled
        ents = {x["path"]: x["value"] for x in trees[0]["entries"]}
        rows, cols = vector_handles(ents["rows"]), vector_handles(ents["cols"])
        root = json.loads(ents["cells"]["contents"])[0]
        part = [[None if rh is None or ch is None else get_cell(root, rh, ch) for ch in cols] for rh in rows[:a.grid_rows]]
        decoded = len(part) * len(cols)
        scale = len(rows) / len(part)
    grid_ms = (time.perf_counter() - t0) * 1e3
    out["python_decode"] = {"json_loads_ms": round(parse_ms, 3), "grid_ms_measured": round(grid_ms, 3), "cells_decoded": decoded,
                            "grid_ms_scaled_to_all_cells": round(grid_ms * scale, 1)}
    print(name, "python_decode", out["python_decode"], flush=True)
    e.close()
    return out


def main():
    from fluidframework_amd import mte
    from tests import matrix_edges as me

    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--grid-rows", type=int, default=16)
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(14)
    out = {"unit": "host clock around one call (plan, upload, kernels, download), ms",
           "batches": {"levels4200": probe(mte, "levels4200", [me.handle_levels().log], a, rng),
                       f"recycle24_x{a.copies}": probe(mte, "recycle24", [me.recycling().log] * a.copies, a, rng)},
           "not_measured": "the host plan's share of a large call (one sort of the probes, the scatter); the kernels alone"}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
