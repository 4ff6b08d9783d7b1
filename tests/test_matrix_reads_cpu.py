"""The SharedMatrix reads without a GPU: the host plan, the CPU build of the walk programs
and the cell-table bodies run as a stand-alone program under ASan and UBSan, and the documents that
tests/test_gpu_matrix_reads.py reads are pinned on the oracle alone to the shapes those tests rely on --
which side of one and two 64-row walk steps each vector's output rows fall, a multi-handle run and a
cleared cell in the recycling document, removed rows still inside the window of the 70-writer one -- so
that a builder change cannot silently move them off a seam."""
import json
import os
import subprocess

import pytest

from tests import matrix_edges as me
from tests.test_matrix_spec import grid

STEP = 64  # output rows one walk step takes (matrix_walk.hpp)
_NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
_PROG = os.path.join(_NATIVE, "_build", "matrix_main")


@pytest.fixture(scope="module")
def docs():
    return {d.name: d for d in me.all_docs()}


@pytest.fixture(scope="module")
def segs(docs):
    """name -> (rows segments, cols segments) of the oracle's final vectors."""
    out = {}
    for n, d in docs.items():
        o = me.oracle(d.log)
        out[n] = (json.loads(o.rows.segments_json()), json.loads(o.cols.segments_json()))
    return out


def test_matrix_plan_walk_and_table_standalone():
    subprocess.run(["make", "-s", "-C", _NATIVE, "-f", "matrix.mk", "_build/matrix_main"], check=True)
    needed = subprocess.run(["ldd", _PROG], check=True, capture_output=True, text=True).stdout
    assert "amdhip" not in needed and "libmte" not in needed, needed
    r = subprocess.run([_PROG], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]  # no failed check, no sanitizer report
    assert r.stdout.startswith("ok: "), r.stdout


def test_row_vectors_span_several_walk_steps(segs):
    """Output rows of every vector the full-grid RECTs walk: the fragmented ones take 22, 6 and 5 steps
    of 64 rows, the spliced ones more than two, the recycling and many-writer ones one (below 64)."""
    want = {"frag1400": 1367, "frag350": 323, "frag300": 269}
    for n, rows in want.items():
        assert len(segs[n][0]) == rows > 2 * STEP and rows % STEP != 0, n
    for n in ("spliced700", "spliced560r"):
        assert len(segs[n][0]) > 2 * STEP, (n, len(segs[n][0]))
    for n in ("recycle24", "writers70", "writers40"):
        assert 1 < len(segs[n][0]) < STEP, (n, len(segs[n][0]))
    # both vectors of the handle-levels matrix cross many steps
    assert len(segs["levels4200"][0]) > 8 * STEP and len(segs["levels4200"][1]) > 8 * STEP


def test_col_vectors_are_narrow(segs, docs):
    """3 or 4 cols where the grids are read whole: a rectangle's row is no multiple of 64 ids, and the
    cols vector is a few output rows (one walk step)."""
    for n in ("frag1400", "frag350", "frag300", "spliced700", "spliced560r", "recycle24", "writers70", "writers40"):
        width = len(docs[n].want_grid[0])
        assert width in (2, 3, 4), (n, width)
        assert 1 <= len(segs[n][1]) < STEP, n
        assert len(docs[n].want_grid) * width % STEP != 0 or n.startswith("writers"), n


def test_recycle24_has_a_run_and_a_cleared_cell(segs, docs):
    d = docs["recycle24"]
    # its final vector holds a run longer than 1, and it is an unallocated one (the re-allocated handles
    # descend, n .. 1, so no two of them coalesce): a probe inside it must not add its offset to 0
    vis = [x for x in segs["recycle24"][0] if "removedSeq" not in x]
    assert max(x["len"] for x in vis) > 1 and all(x["len"] == 1 for x in vis if x["start"] != me.UNALLOC), vis
    assert sorted(x["len"] for x in vis if x["start"] == me.UNALLOC) == [1, 2]
    # (the allocated runs longer than 1, handle = start + offset, are the handle-levels matrix's rows)
    lv = [x["len"] for x in segs["levels4200"][0] if "removedSeq" not in x and x["start"] != me.UNALLOC]
    assert max(lv) > 1 and sum(lv) == 4200, max(lv)
    # a cell the UNLINK cleared and no later set wrote again, on an allocated (row, col) pair
    s = json.loads(me.oracle(d.log).snapshot_json())
    g, h = grid(s), me.handles(s)
    assert g == d.want_grid
    cleared = [(r, c) for r, row in enumerate(g) for c, v in enumerate(row)
               if v is None and h["rows"][r] is not None and h["cols"][c] is not None]
    assert cleared, g


def test_writers70_has_removed_rows_inside_the_window(segs):
    """Output rows that are removed but still inside the collaboration window (length 0 in the local view):
    the removed col of the 70-writer matrix, between visible ones (its removed ROWS are all unlinked by the
    tail), and the 20 removed rows of the 700-row spliced vector, past its eighth 64-row step."""
    cols = segs["writers70"][1]
    gone = [i for i, x in enumerate(cols) if "removedSeq" in x]
    assert gone and 0 < gone[0] and gone[-1] < len(cols) - 1, (gone, len(cols))
    assert not any("removedSeq" in x for x in segs["writers70"][0])
    rows = segs["spliced700"][0]
    gone = [i for i, x in enumerate(rows) if "removedSeq" in x]
    assert len(gone) == 20 and gone[0] > 8 * STEP and gone[-1] < len(rows) - 1, (gone, len(rows))


def test_big_summary_rows_named_by_the_builder():
    """The rows the GPU test reads in the 65 600-handle matrix: the builder's expectation names cells
    either side of handle 65 536 and a cleared loaded pair."""
    _, _, want = me.big_handle_summary()
    rows = sorted({rh for rh, _ in want["cells"]})
    assert any(rh < 65536 for rh in rows) and any(rh >= 65536 for rh in rows)
    assert (65535, 2) not in want["cells"] and (65536, 3) not in want["cells"]
