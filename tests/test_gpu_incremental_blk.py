"""GPU: incremental replay of the documents the row engines cannot hold (mte_retain; engine.hpp
Engine::ckpt_save / ckpt_resume, mte_ckpt.hip k_blk_ck). Documents loaded from a summary, with relative
positions, or with 64 or more clients in the window run on the block engine; on a retained pass each
leaves a block checkpoint, and a pass over a log that extends the last one continues from it. Every
pass is compared with the oracle fed the same messages, and the counters (resumed_docs_blk,
resumed_ops_blk) show the pass did not replay the old op records again."""
import ctypes
import functools
import random

import pytest

from fluidframework_amd import mte
from oracle import OracleDoc
from tests.catchup import OBS, c5_json_log, catchup_cases
from tests.gpu_helpers import compare_batch_checksums, compare_doc
from tests.oplog import dumps, ins, msg, rem

pytestmark = pytest.mark.gpu


def _text(engine_text):
    # (the oracle's Python text is UTF-8: lone surrogates compare in the same form, gpu_helpers.py)
    return engine_text.encode("utf-16-le", "surrogatepass").decode("utf-16-le", "replace")


def _n_records(builder, d=0):
    bt = builder.batch()
    return bt.doc_op_offsets[d + 1] - bt.doc_op_offsets[d]


@pytest.mark.parametrize("seed", [0, 1])
def test_summary_loaded_client_reads_incrementally(seed):
    """MergeTreeClient.load(summary) (a header-only SnapshotV1 summary of a 1 500-message log cut at a
    random message), then the suffix with reads at five random cuts and at its end: every read equals
    the oracle client that loaded the same summary and applied the same messages, and every read after
    the first went on from the previous read's op records (the summary's LOAD records included)."""
    summary, suffix, _ = catchup_cases(1, 1500, seed=seed, chunk=10000)[0]
    rng = random.Random(seed)
    cuts = sorted(rng.sample(range(1, len(suffix)), 5)) + [len(suffix)]
    c = mte.MergeTreeClient(OBS)
    c.load(summary)
    o = OracleDoc(OBS)
    assert o.load_summary(summary) == 0, o.status()
    at, prev_records = 0, 0
    for k, cut in enumerate(cuts):
        for m in suffix[at:cut]:
            c.applyMsg(m)
        assert o.apply_json(dumps(suffix[at:cut])) == 0, o.status()
        assert _text(c.getText()) == o.text(), f"read {k} after {cut} messages"
        assert c.getLength() == o.length()
        e = c._engine
        assert e.segments_json(0) == o.segments_json(), f"read {k}"
        assert e.snapshot_json(0) == o.snapshot_json(), f"read {k}"
        print(f"seed {seed} read {k}: resumed_docs_blk {e.get_info('resumed_docs_blk')} resumed_ops {c.resumed_ops()} "
              f"previous records {prev_records} saved {e.get_info('ck_blk_saved')}")
        if k:
            assert e.get_info("resumed_docs_blk") == 1
            assert c.resumed_ops() == prev_records, (k, cut, c.resumed_ops(), prev_records)
        else:
            assert e.get_info("resumed_docs_blk") == 0 and c.resumed_ops() == 0
        assert e.get_info("ck_blk_saved") == 1 and e.get_info("resumed_docs") == 0
        prev_records = _n_records(c._builder)
        at = cut
    assert c.replays == len(cuts)


def _three_passes(docs, observer, fracs=None, cuts=None, adder="add_doc"):
    """One retained engine over three batches of growing logs (a fresh Builder per pass). docs: per
    document its messages (add_doc) or (summary, suffix) (add_doc_from_summary); the cut of pass i is
    fracs[i] of each log or cuts[d][i]. Yields (pass, engine, batch) after each replay."""
    e = mte.Engine(0)
    e.retain(True)
    try:
        for i in range(3):
            b = mte.Builder()
            for d, doc in enumerate(docs):
                log = doc[1] if adder == "summary" else doc
                k = cuts[d][i] if cuts else (len(log) if fracs[i] == 1.0 else max(1, int(len(log) * fracs[i])))
                if adder == "summary":
                    b.add_doc_from_summary(doc[0], log[:k], observer=observer)
                else:
                    b.add_doc(log[:k], observer=observer)
            bt = b.batch()
            e.load(bt)
            e.replay()
            yield i, e, bt
    finally:
        e.close()


def test_body_chunk_summaries_with_merge_info_resume():
    """Summaries whose body chunks hold merge-info segments (LOAD_APPEND records), each with a third,
    two thirds and all of its suffix: passes 2 and 3 continue all four documents."""
    from tests.test_summary_load import OBS as SOBS, collab_body_summaries

    cases = [collab_body_summaries()[i] for i in (1, 2, 4, 5)]
    cuts = [(len(s) // 3, 2 * len(s) // 3, len(s)) for _, s in cases]
    for i, e, bt in _three_passes(cases, SOBS, cuts=cuts, adder="summary"):
        for d in range(len(cases)):
            compare_doc(e, bt, d, observer=SOBS)
        print("pass", i, {k: e.get_info(k) for k in ("ck_offered", "resumed_docs_blk", "resumed_ops_blk", "ck_blk_saved")})
        assert e.get_info("ck_blk_saved") == 4
        assert e.get_info("resumed_docs_blk") == (4 if i else 0)
        if i:
            assert e.get_info("resumed_ops_blk") == sum(prev)
        prev = [bt.doc_op_offsets[d + 1] - bt.doc_op_offsets[d] for d in range(len(cases))]


@functools.lru_cache(maxsize=None)
def _relative_docs():
    from tests.test_relative_pos import relative_log

    return [relative_log(s, n=600) for s in (0, 1, 2)] + [c5_json_log(700 + i, 300) for i in range(8)]


def test_relative_positions_beside_row_documents_in_one_growing_builder():
    """Three documents with relative positions (block documents) beside eight the row engines hold, all
    open documents of ONE builder grown by append (so the interned property tables of each pass extend
    the last pass's): in passes 2 and 3 every log is offered its checkpoint, the eight continue from
    row checkpoints and the three from block checkpoints."""
    docs = _relative_docs()
    e = mte.Engine(0)
    try:
        e.retain(True)
        b = mte.Builder()
        ids = [b.open_doc(OBS) for _ in docs]
        at = [0] * len(docs)
        for i, frac in enumerate((0.4, 0.7, 1.0)):
            for d, l in enumerate(docs):
                k = len(l) if frac == 1.0 else max(1, int(len(l) * frac))
                b.append(ids[d], l[at[d]:k])
                at[d] = k
            bt = b.batch()
            e.load(bt)
            e.replay()
            bad, _, _ = compare_batch_checksums(e, bt)
            assert not bad, (i, bad)
            for d in range(3):
                compare_doc(e, bt, d, observer=OBS)
            info = {k: e.get_info(k) for k in ("ck_offered", "resumed_docs", "resumed_docs_blk", "ck_blk_saved", "rows")}
            print("pass", i, info)
            if i:
                assert info["ck_offered"] == 11, info
                assert info["resumed_docs"] == 8 and info["resumed_docs_blk"] == 3, info
            else:
                assert info["resumed_docs"] == 0 and info["resumed_docs_blk"] == 0, info
            assert info["ck_blk_saved"] == 3, info
    finally:
        e.close()


def test_relative_positions_beside_row_documents():
    """Three documents with relative positions (block documents) beside eight the row engines hold, a
    fresh Builder per pass: in passes 2 and 3 every log extends the last pass's (ck_offered), the eight
    continue from row checkpoints and the three from block checkpoints.

    The three documents carry properties (marker ids, annotates), and a fresh Builder interns keys and
    values document by document, so the tables of a pass with longer logs do not start with the last
    pass's: the prefix check hashes property sets by content, and the kept block checkpoints' map
    records are renumbered to the loaded batch's ids (engine_run.cpp ck_match_batch, k_ck_xlate). The
    segment tables compared below carry those properties."""
    docs = _relative_docs()
    for i, e, bt in _three_passes(docs, OBS, fracs=(0.4, 0.7, 1.0)):
        bad, _, _ = compare_batch_checksums(e, bt)
        assert not bad, (i, bad)
        for d in range(3):
            compare_doc(e, bt, d, observer=OBS)
        info = {k: e.get_info(k) for k in ("ck_offered", "resumed_docs", "resumed_docs_blk", "ck_blk_saved", "rows")}
        print("pass", i, info)
        if i:
            # first: the builder reproduced every prefix (else nothing was offered to resume from)
            assert info["ck_offered"] == 11, info
            assert info["resumed_docs"] == 8 and info["resumed_docs_blk"] == 3, info
        else:
            assert info["resumed_docs"] == 0 and info["resumed_docs_blk"] == 0, info
        assert info["ck_blk_saved"] == 3, info


def test_windows_of_64_or_more_clients_resume_with_their_overlap_masks():
    """70 concurrent writers, and 100 writers whose removes all overlap: every cut already has more
    than 64 clients in the window, so removedClientOverlap of clients 64..127 (ovl2) is part of the
    state saved and restored. The full segment tables (overlap lists) equal the oracle's each pass."""
    from tests.test_many_clients import OBS as MOBS, concurrent_log, overlap_log

    docs = [concurrent_log(70, 400), overlap_log(100)]
    assert len(docs[1]) >= 232
    cuts = [(200, 300, 400), (120, 180, 232)]
    for i, e, bt in _three_passes(docs, MOBS, cuts=cuts):
        for d in range(2):
            compare_doc(e, bt, d, observer=MOBS)
        info = {k: e.get_info(k) for k in ("ck_offered", "resumed_docs_blk", "resumed_ops_blk", "ck_blk_saved")}
        print("pass", i, info)
        assert info["resumed_docs_blk"] == (2 if i else 0), info
        assert info["ck_blk_saved"] == 2, info


@functools.lru_cache(maxsize=None)
def _fixed_rows_logs(kind):
    """The 64 documents of tests/test_gpu_reg.py's fixed-rows case (generate(kind, 64, 6000, 8 writers,
    seed 31): a document's log depends only on its id, op count, kind, writers and seed), as messages."""
    from bench import ops_to_messages
    from tests import regcpu

    logs = []
    for d in range(64):
        ops, pay = regcpu.generated(kind, d, 6000, n_clients=8, seed=31)
        logs.append(ops_to_messages(ops, pay, 0, len(ops)))
    return logs


@pytest.mark.parametrize("kind", [2, 5])
def test_documents_that_leave_their_rows_mid_pass_continue_on_the_block_engine(kind):
    """reg_lb_limit = 24 makes k_rows documents outgrow their rows between two ops and finish
    HBM-resident in the pass (k_rows_cont, DocRes mode 6). With retain on each of them leaves a block
    checkpoint there, and on the next pass, over the whole logs, it is a block document that k_blk_ck
    continues; every other document continues from its row checkpoint."""
    logs = _fixed_rows_logs(kind)
    e = mte.Engine(0)
    try:
        e.retain(True)
        e.set_option("reg_lb_limit", 24)
        n6 = None
        for i, frac in enumerate((0.6, 1.0)):
            b = mte.Builder()
            for l in logs:
                b.add_doc(l if frac == 1.0 else l[:int(len(l) * frac)])
            bt = b.batch()
            e.load(bt)
            st = e.replay()
            info = e.run_info()
            modes = [e.doc_result(d)["mode"] for d in range(len(logs))]
            ck = {k: e.get_info(k) for k in ("ck_offered", "resumed_docs", "resumed_docs_blk", "resumed_ops_blk", "ck_blk_saved")}
            print("kind", kind, "pass", i, "rows_continued", info["rows_continued"], "spilled", info["spilled"],
                  "modes", {m: modes.count(m) for m in sorted(set(modes))}, ck)
            assert st["failed_docs"] == 0
            bad, _, _ = compare_batch_checksums(e, bt)
            assert not bad, (i, bad)
            if i == 0:
                assert info["rows_continued"] > 0, info
                n6 = modes.count(6)
                assert n6 == info["rows_continued"], (modes, info)
                assert ck["ck_blk_saved"] == n6, ck
                prev = [bt.doc_op_offsets[d + 1] - bt.doc_op_offsets[d] for d in range(len(logs))]
                was6 = [m == 6 for m in modes]
            else:
                assert ck["resumed_docs_blk"] == n6, ck
                assert ck["resumed_docs"] + ck["resumed_docs_blk"] == len(logs), ck
                assert ck["resumed_ops_blk"] == sum(p for p, w in zip(prev, was6) if w), ck
                assert all(modes[d] == 1 for d in range(len(logs)) if was6[d]), modes
    finally:
        e.set_option("reg_lb_limit", 0)
        e.close()


def _long_relative_log(n):
    """A relative_log-style document of n messages: 200 messages with relative positions, then one
    writer inserting and removing at the front of its own up-to-date view."""
    from tests.test_relative_pos import relative_log

    msgs = relative_log(7, n=200)
    o = OracleDoc(OBS)
    assert o.apply_json(dumps(msgs)) == 0
    rng = random.Random(5)
    length = o.length()
    for seq in range(len(msgs) + 1, n + 1):
        if length > 4 and rng.random() < 0.4:
            k = rng.randint(1, 3)
            contents = rem(0, k)
            length -= k
        else:
            t = "".join(rng.choice("uvw") for _ in range(rng.randint(1, 5)))
            contents = ins(0, t)
            length += len(t)
        msgs.append(msg("a", seq, seq - 1, contents, seq - 1))
    return msgs


def test_document_over_the_budget_is_skipped():
    """ck_blk_budget_mb = 1: the block region of a 20 000-message document with relative positions
    does not fit, so it is not listed, leaves no checkpoint and replays from op 0 on the next pass --
    with the oracle's results both times."""
    msgs = _long_relative_log(20_000)
    e = mte.Engine(0)
    try:
        e.retain(True)
        e.set_option("ck_blk_budget_mb", 1)
        for i, cut in enumerate((15_000, 20_000)):
            b = mte.Builder()
            b.add_doc(msgs[:cut], observer=OBS)
            bt = b.batch()
            e.load(bt)
            e.replay()
            info = {k: e.get_info(k) for k in ("ck_offered", "ck_blk_skipped", "resumed_docs_blk", "ck_blk_saved", "resumed_docs")}
            print("pass", i, info)
            assert info["ck_blk_skipped"] == 1 and info["ck_blk_saved"] == 0, info
            assert info["resumed_docs_blk"] == 0 and info["resumed_docs"] == 0, info
            assert e.status(0)[0] == 0
            compare_doc(e, bt, 0, observer=OBS)
    finally:
        e.set_option("ck_blk_budget_mb", 1024)
        e.close()


def test_retain_off_then_on():
    """Without retain nothing is kept or resumed; the first retained pass starts from op 0, the next
    continues every block document, and retain(False) drops the state again: the same batch's results
    are the same every time."""
    docs = _relative_docs()[:3]
    e = mte.Engine(0)
    try:
        b = mte.Builder()
        for l in docs:
            b.add_doc(l[:400], observer=OBS)
        bt = b.batch()
        e.load(bt)
        e.replay()
        first = e.summaries()["checksum"].copy()
        bad, _, _ = compare_batch_checksums(e, bt)
        assert not bad, bad
        e.replay()
        assert e.get_info("resumed_docs_blk") == 0 and e.get_info("ck_blk_saved") == 0
        e.retain(True)
        e.replay()  # (nothing kept yet)
        assert e.get_info("resumed_docs_blk") == 0 and e.get_info("ck_blk_saved") == 3
        assert (e.summaries()["checksum"] == first).all()
        e.replay()
        assert e.get_info("resumed_docs_blk") == 3
        assert e.get_info("resumed_ops_blk") == bt.doc_op_offsets[3]
        assert (e.summaries()["checksum"] == first).all()
        for d in range(3):
            compare_doc(e, bt, d, observer=OBS)
        e.retain(False)
        e.replay()
        assert e.get_info("resumed_docs_blk") == 0 and e.get_info("resumed_ops_blk") == 0
        assert (e.summaries()["checksum"] == first).all()
    finally:
        e.close()
