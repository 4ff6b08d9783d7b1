"""GPU: a retained pass (mte_retain) with both per-pass property-map tables alive: documents the host
re-runs HBM-resident (rerun_spilled: the re-run's worst-case table) beside block documents on k_blk_ck
(their own worst-case table), all of them carrying annotates. Both routes overwrite DocCfg::map_off /
map_cap for the pass and put the load-time values back; the next pass, over longer logs, starts from
them again. Every document is compared with the oracle after each pass."""
import random

import pytest

from fluidframework_amd import mte
from tests.catchup import OBS
from tests.gpu_helpers import compare_batch_checksums, compare_doc
from tests.oplog import ann, ins, msg, rem

pytestmark = pytest.mark.gpu


def annotated_log(seed, n):
    """Three writers, each up to date (refSeq = seq - 1): inserts, removes and annotates at positions
    of the current text; the annotates' values keep neighbouring segments from merging."""
    rng = random.Random(seed)
    msgs, length = [], 0
    for seq in range(1, n + 1):
        r = rng.random()
        if length > 8 and r < 0.2:
            a = rng.randrange(length - 3)
            k = rng.randint(1, 3)
            contents = rem(a, a + k)
            length -= k
        elif length > 8 and r < 0.5:
            a = rng.randrange(length - 3)
            contents = ann(a, a + rng.randint(1, 3), {rng.choice(["b", "i"]): rng.choice([True, None, 3, 4, 5])})
        else:
            t = "".join(rng.choice("abcdef") for _ in range(rng.randint(1, 5)))
            contents = ins(rng.randint(0, length), t)
            length += len(t)
        msgs.append(msg("abc"[seq % 3], seq, seq - 1, contents, max(0, seq - 20)))
    return msgs


def test_host_rerun_beside_block_documents_on_a_retained_pass():
    """Three documents with relative positions (block documents of a retained pass) and eight the row
    engines could hold, forced HBM-resident into slots of 8 leaf blocks (force_hbm, slot_blk_limit, as
    tests/test_relative_pos.py forces a re-run), which they outgrow: the host re-runs them. Two passes,
    60 % of every log and then all of it, a fresh Builder each: both routes ran in each pass, the block
    documents continue from their checkpoints in the second, and text, segments with their property
    maps, SnapshotV1 and the summary checksums of all eleven documents equal the oracle's both times."""
    from tests.test_gpu_incremental_blk import _relative_docs

    docs = list(_relative_docs()[:3]) + [annotated_log(40 + i, 300) for i in range(8)]
    e = mte.Engine(0)
    try:
        e.retain(True)
        e.set_option("slot_blk_limit", 8)
        saved = None
        for i, frac in enumerate((0.6, 1.0)):
            b = mte.Builder()
            for l in docs:
                b.add_doc(l if frac == 1.0 else l[:int(len(l) * frac)], observer=OBS)
            bt = b.batch()
            e.load(bt)
            e.set_option("force_hbm", 1)
            st = e.replay()
            info = e.run_info()
            ck = {k: e.get_info(k) for k in ("ck_offered", "resumed_docs", "resumed_docs_blk", "ck_blk_saved", "ck_blk_skipped")}
            print("pass", i, "spilled", info["spilled"], ck)
            # both routes ran, each with a map table of its own
            assert info["spilled"] >= 1, info
            assert ck["ck_blk_saved"] >= 1, ck
            if i:
                assert ck["resumed_docs_blk"] == saved, ck
            saved = ck["ck_blk_saved"]
            assert st["failed_docs"] == 0, st
            bad, _, _ = compare_batch_checksums(e, bt)
            assert not bad, (i, bad)
            for d in range(len(docs)):
                compare_doc(e, bt, d, observer=OBS)
    finally:
        e.set_option("force_hbm", 0)
        e.set_option("slot_blk_limit", 0)
        e.close()
