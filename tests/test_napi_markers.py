"""The marker queries through the N-API addon (packages/merge-tree-native/test/markers.gpu.js): markers()
of BatchedMergeEngine on the seam document and a random log, and MergeTreeClient's findTile /
getTextAndMarkers, compared with tests/markers.py on the oracle's tables."""
import json
import os
import random
import shutil
import subprocess

import pytest

from oracle import OracleDoc
from tests import markers
from tests.markers import PARAGRAPHS, TILE_AFTER, TILE_BEFORE, TO_END, Writer, text_seg, tile
from tests.oplog import dumps
from tests.test_gpu_fuzz import random_json_log
from tests.views import rows_of, units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "packages", "merge-tree-native")
ADDON = os.path.join(PKG, "build", "mte_native.node")

node = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason="node not installed")]


def table(log):
    o = OracleDoc(markers.OBSERVER)
    o.apply_json(dumps(log))
    assert o.status()[0] == 0
    return rows_of(o)


def test_markers_through_the_addon(tmp_path):
    if not os.path.exists(ADDON):
        subprocess.run(["make", "-s", "-C", PKG], check=True)
    w = Writer()
    for i, (pos, seg) in enumerate([(0, tile(markerId="m0")), (0, "abc d"), (0, tile(markerId="m1")), (7, "ef"),
                                    (8, tile(markerId="m2")), (10, text_seg("bold", bold="bold")), (14, tile(markerId="m3"))]):
        w.insert(pos, seg)
    logs = [markers.seam_log(), markers.tiled(random_json_log(21, 300, n_writers=8, emoji=True), 21), w.log]
    tables = [table(log) for log in logs]
    labels = ["EOP", "H1", "\U0001F600"]
    rng = random.Random(3)
    q = []
    for d, rows in enumerate(tables):
        L = sum(markers.net_len(r) for r in rows)
        for _ in range(100):
            q.append((d, rng.choice([TILE_BEFORE, TILE_AFTER]), rng.randint(0, L + 2), 0, rng.randrange(3)))
        q += [(d, PARAGRAPHS, 0, TO_END, li) for li in range(3)]
        q += [(d, PARAGRAPHS, a, a + n, 0) for a, n in ((1, 0), (3, 40), (L // 2, 1000))]
    probes = list(range(17))
    inp = {"observer": markers.OBSERVER, "logs": logs, "facade": w.log, "facadeLabel": "EOP", "facadeProbes": probes,
           "queries": [{"doc": d, "kind": k, "pos1": a, "pos2": b, "label": labels[li]} for d, k, a, b, li in q]}
    path = tmp_path / "markers_in.json"
    path.write_text(json.dumps(inp))
    r = subprocess.run([node, os.path.join(PKG, "test", "markers.gpu.js"), str(path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["downloaded"] == 0 and len(out["results"]) == len(q)
    for got, (d, k, a, b, li) in zip(out["results"], q):
        want = markers.expect(tables[d], k, a, b, labels[li])
        assert got["status"] == want["status"], (got, want)
        if k == PARAGRAPHS:
            assert [(p["row"], p["pos"], units(p["text"])) for p in got["pieces"]] == \
                [(p["row"], p["pos"], p["units"]) for p in want["pieces"]], (got, want)
        elif want["status"] == markers.OK:
            assert (got["row"], got["pos"], got["removed"]) == (want["row"], want["pos"], bool(want["flags"])), (got, want)
    f = out["facade"]
    rows = tables[2]

    def tile_of(t):
        return None if t is None else {"pos": t[1], "row": t[0]}

    assert f["before"] == [tile_of(markers.find_tile(rows, p, "EOP")) for p in probes]
    assert f["after"] == [tile_of(markers.find_tile(rows, p, "EOP", False)) for p in probes]
    assert f["paragraphs"]["parallelText"] == ["", "abc d", "e", "f<b>bold"]
    assert [(m["pos"], m["properties"]["markerId"]) for m in f["paragraphs"]["parallelMarkers"]] == \
        [(0, "m1"), (6, "m0"), (8, "m2"), (14, "m3")]
