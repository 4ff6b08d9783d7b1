"""The N-API MergeTreeClient after load(summary) reads incrementally (packages/merge-tree-native/test/
incremental.gpu.js): resumedOps() counts the op records the block engine continued past."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "packages", "merge-tree-native")
ADDON = os.path.join(PKG, "build", "mte_native.node")

node = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason="node not installed")]


def test_client_loaded_from_a_summary_reads_incrementally():
    if not os.path.exists(ADDON):
        subprocess.run(["make", "-s", "-C", PKG], check=True)
    r = subprocess.run([node, os.path.join(PKG, "test", "incremental.gpu.js")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["reads"] == 6 and out["resumed"][0] == 0 and all(x > 0 for x in out["resumed"][1:]), out
