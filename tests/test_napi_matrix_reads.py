"""The SharedMatrix reads through the N-API addon (packages/merge-tree-native/test/matrix.gpu.js):
matrixCells() and valueText() of BatchedMergeEngine on one matrix.spec.ts conflict case and on the
recycling document of tests/matrix_edges.py, compared with the oracle's grid and handles."""
import json
import os
import shutil
import subprocess

import pytest

from tests import matrix_edges as me
from tests.test_matrix_spec import CASES, build, grid, oracle_summary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "packages", "merge-tree-native")
ADDON = os.path.join(PKG, "build", "mte_native.node")
OK, OUT_OF_RANGE = 0, 1

node = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason="node not installed")]


def test_matrix_cells_through_the_addon(tmp_path):
    if not os.path.exists(ADDON):
        subprocess.run(["make", "-s", "-C", PKG], check=True)
    spec_log, spec_grid = build(CASES["overlapping insert/set vs. remove/insert/set (600)"])
    rec = me.recycling()
    logs = [spec_log, rec.log]
    path = tmp_path / "matrix_in.json"
    path.write_text(json.dumps({"observer": "observer", "matrices": logs}))
    r = subprocess.run([node, os.path.join(PKG, "test", "matrix.gpu.js"), str(path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["downloaded"] == 0 and out["built"] == 2 and out["nullText"] == "null"
    for got, log, closed in zip(out["matrices"], logs, (spec_grid, rec.want_grid)):
        tree = oracle_summary(log)
        want, h = grid(tree), me.handles(tree)
        assert want == closed
        assert (got["rowCount"], got["colCount"]) == (len(want), len(want[0]))
        assert got["status"] == [OK, OK, OK, OUT_OF_RANGE, OUT_OF_RANGE]
        assert got["grid"] == want
        assert got["first"] == want[0][0] and got["last"] == want[-1][-1]
        assert got["handles"] == [h["rows"][0] or 0, h["cols"][0] or 0, h["rows"][-1] or 0, h["cols"][-1] or 0]
        assert got["outside"] == [[None]] * len(want)   # rows 1 .. rowCount: one past the end, all undefined
