"""Per-read replay time of a client that starts from a summary (option retain, block checkpoints):
c5_json_log(1, 10 000) summarized by the oracle at message 2 000, then the suffix read every 500
messages on one retained engine (a fresh Builder with add_doc_from_summary(summary, suffix so far) per
read, which every build of the library accepts). Prints mte_last_kernel_ms and the resume counters of
each read.

  python tools/incremental_blk_probe.py                      this build, one series, one JSON line
  python tools/incremental_blk_probe.py --ab OTHER --out F   this build and fluidframework_amd/_build/OTHER/
      libmte.so (say, the parent commit's library) alternating, each series in a fresh process
      (MTE_LIB selects the library at import), twice each; both series of every run go to F."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def series():
    from fluidframework_amd import mte
    from oracle import OracleDoc
    from tests.catchup import OBS, c5_json_log
    from tests.oplog import dumps

    log = c5_json_log(1, 10_000)
    o = OracleDoc(OBS)
    assert o.apply_json(dumps(log[:2000])) == 0
    summary, suffix = o.snapshot_json(10000), log[2000:]
    e = mte.Engine(0)
    e.retain(True)
    reads = []
    for k in range(500, len(suffix) + 1, 500):
        b = mte.Builder()
        b.add_doc_from_summary(summary, suffix[:k], observer=OBS)
        bt = b.batch()
        e.load(bt)
        e.replay()
        assert e.status(0)[0] == 0, e.status(0)
        r = {"messages": 2000 + k, "records": int(bt.doc_op_offsets[1]), "kernel_ms": round(e.last_kernel_ms(), 3)}
        for key in ("resumed_docs", "resumed_ops", "resumed_docs_blk", "resumed_ops_blk"):
            try:
                r[key] = e.get_info(key)
            except mte.MteError:  # (a build from before the block checkpoints)
                pass
        reads.append(r)
    o.apply_json(dumps(suffix))
    assert e.text(0) == o.text()
    e.close()
    return reads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", help="another build under fluidframework_amd/_build/ to alternate with")
    ap.add_argument("--out", help="JSON file for the series")
    a = ap.parse_args()
    if not a.ab:
        print(json.dumps({"lib": os.environ.get("MTE_LIB", ""), "reads": series()}))
        return
    runs = []
    for rep in range(2):
        for lib in ("", a.ab):
            env = dict(os.environ, MTE_LIB=lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode:
                sys.exit(f"series on '{lib or 'this build'}' failed:\n{r.stderr[-2000:]}")
            runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(lib or "this build", [x["kernel_ms"] for x in runs[-1]["reads"]], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"workload": "c5_json_log(1, 10000), summary at message 2000, a read every 500 messages",
                       "unit": "mte_last_kernel_ms per read", "runs": runs}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
