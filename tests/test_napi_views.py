"""The view queries through the N-API addon (packages/merge-tree-native/test/views.gpu.js): views(),
clientSlot() and viewProps() of BatchedMergeEngine on the SharedString spec's annotate case and a random
log, and MergeTreeClient's positional reads, compared with tests/views.py on the oracle's tables."""
import json
import os
import random
import shutil
import subprocess

import pytest

from oracle import OracleDoc
from tests import views
from tests.oplog import dumps
from tests.test_gpu_fuzz import random_json_log
from tests.test_sharedstring_spec import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "packages", "merge-tree-native")
ADDON = os.path.join(PKG, "build", "mte_native.node")

node = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason="node not installed")]


def test_views_through_the_addon(tmp_path):
    if not os.path.exists(ADDON):
        subprocess.run(["make", "-s", "-C", PKG], check=True)
    spec = CASES["annotate"][0]
    logs = [spec, random_json_log(21, 300, n_writers=8, emoji=False)]
    tables = []
    for log in logs:
        o = OracleDoc(views.OBSERVER)
        o.apply_json(dumps(log))
        assert o.status()[0] == 0
        tables.append(views.rows_of(o))
    rng = random.Random(3)
    names = sorted({m["clientId"] for m in logs[1]})
    msn = logs[1][-1]["minimumSequenceNumber"]
    q = [(0, 0, views.OBSERVER, k, a, b) for k in (0, 1, 2) for a, b in ((0, 11), (6, 11), (11, 12), (3, 3))]
    q += [(0, 2, "s1", views.LOCATE, p, 0) for p in range(12)]
    for _ in range(300):
        p1 = rng.randint(0, 400)
        q.append((1, rng.randint(msn, len(logs[1])), rng.choice(names + [views.OBSERVER, None]), rng.randint(0, 2), p1,
                  p1 + rng.choice([0, 3, 50, 5000])))
    inp = {"observer": views.OBSERVER, "logs": logs, "facade": spec,
           "queries": [{"doc": d, "refSeq": r, "client": "" if c == views.OBSERVER else c, "kind": k, "pos1": a, "pos2": b}
                       for d, r, c, k, a, b in q]}
    path = tmp_path / "views_in.json"
    path.write_text(json.dumps(inp))
    r = subprocess.run([node, os.path.join(PKG, "test", "views.gpu.js"), str(path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["downloaded"] == 0 and out["noSlot"] is True
    assert len(out["results"]) == len(q)
    for got, (d, ref, c, k, a, b) in zip(out["results"], q):
        want = views.View(tables[d], ref, c).expect(k, a, b)
        assert got["status"] == want["status"] and got["length"] == want["length"], (got, want)
        if k == views.LOCATE and want["status"] == views.OK:
            assert (got["row"], got["offset"], got["curPos"], got["removed"]) == \
                (want["row"], want["offset"], want["cur_pos"], bool(want["flags"])), (got, want)
        if k == views.TEXT:
            assert views.units(got["text"]) == want["units"], (got, want)
    bold, both = {"style": "bold"}, {"style": "bold", "color": "green"}
    assert out["rows"] == [bold, both]
    f = out["facade"]
    assert f["props"] == [bold] * 6 + [both] * 5 + [None]
    assert f["segment"] == [[0, p] for p in range(6)] + [[1, p] for p in range(5)] + [None]
    assert f["position"] == [0, 6] and f["text"] == "world" and f["tail"] == "world" and f["all"] == "hello world"
    assert f["lengthAt"] == 11 and f["past"] == {}
