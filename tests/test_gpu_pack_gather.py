"""GPU: the fused pack (reg_engine.hpp pack_fused: a pack's siblings decided at once from row-wide masks,
the kept slots gathered by keep mask) against the oracle -- status, text, segment table and SnapshotV1
bytes (tests/gpu_helpers.py compare_doc). On k_solo: lean with siblings in two rows and cascades, kind 5
(zamboni after nearly every op), PROPS + WIDE with properties, 33 writers, the hand-written log whose
popped block joins across the tombstone its first scour dropped, and the long inserts whose packs go back
to the sibling loop for the serial walk. On k_rows at 4 and 12 waves (fixed quarters, the paged pool): 48
documents of kinds 2 / 3 / 5, whether or not the fused path is built into those engines. The shapes are
the smallest at which each path occurs; tests/test_reg_pack_gather_cpu.py asserts by counter, on the CPU
build, that every document here reaches its shape.

The arena_gc fallback has no device knob (the host sizes a document's arena from its payload): it is
covered on the CPU build only (test_arena_gc_hands_the_pack_back)."""
import pytest

from fluidframework_amd import mte
from tests.gpu_helpers import compare_batch_checksums, compare_doc
from tests.oplog import dumps
from tests.pack_gather_docs import SOLO_DOCS, long_insert_log, tombstone_log

pytestmark = pytest.mark.gpu

MODE_ROWS, MODE_BULK_ROWS = 4, 5


@pytest.fixture(scope="module")
def engine():
    e = mte.Engine(0)
    e.set_option("solo_min_ops", 1)  # one-document batches take the solo route
    yield e
    e.set_option("rows_bulk", -1)
    e.close()


@pytest.mark.parametrize("kind,n_ops,clients,gid,seed", SOLO_DOCS)
def test_generated_document_on_k_solo(engine, kind, n_ops, clients, gid, seed):
    engine.set_option("rows_bulk", -1)
    engine.generate(kind, 1, n_ops, n_clients=clients, seed=seed, doc_ids=[gid])
    batch = engine.export_batch()
    st = engine.replay()
    r = engine.doc_result(0)
    assert engine.run_info()["solo"] == 1 and r["status"] == 0 and st["ops"] == n_ops and r["mode"] == MODE_ROWS, r
    if kind == 2 and clients == 8:
        assert r["max_lb"] > 8, r  # a second row
    compare_doc(engine, batch, 0)


@pytest.mark.parametrize("log", [tombstone_log, long_insert_log])
def test_hand_made_log_on_k_solo(engine, log):
    """Through the Builder: the tombstone log (the popped block changes in the pack's own pass) and the
    long inserts (packs handed back for the serial walk, on the device)."""
    engine.set_option("rows_bulk", -1)
    b = mte.Builder()
    b.add_doc(dumps(log()))
    batch = b.batch()
    engine.load(batch)
    engine.replay()
    r = engine.doc_result(0)
    assert engine.run_info()["solo"] == 1 and r["status"] == 0 and r["mode"] == MODE_ROWS, r
    compare_doc(engine, batch, 0)


@pytest.mark.parametrize("waves", [4, 12])
@pytest.mark.parametrize("kind,n_ops", [(2, 3000), (3, 2000), (5, 2000)])
def test_documents_on_k_rows(engine, kind, n_ops, waves):
    """48 bulk documents on k_rows: every checksum against the oracle, the first two in full."""
    engine.set_option("rows_bulk", waves)
    try:
        engine.generate(kind, 48, n_ops, n_clients=8, seed=1000)
        batch = engine.export_batch()
        st = engine.replay()
        assert st["failed_docs"] == 0 and engine.get_info("rows") == waves, engine.run_info()
        modes = [engine.doc_result(d)["mode"] for d in range(48)]
        assert modes.count(MODE_BULK_ROWS) >= 48 - 16, (modes, engine.run_info())
        bad, _, _ = compare_batch_checksums(engine, batch, threads=16)
        for d in sorted(set(bad[:1] + [0, 1])):
            compare_doc(engine, batch, d)
        assert not bad
    finally:
        engine.set_option("rows_bulk", -1)


def test_double_replay_gives_equal_bytes(engine):
    """One batch replayed twice (k_solo, then again on the same engine): equal summaries, segment tables
    and snapshots."""
    engine.set_option("rows_bulk", -1)
    engine.generate(2, 1, 3000, n_clients=8, seed=17, doc_ids=[1])
    got = []
    for _ in range(2):
        engine.replay()
        got.append((engine.summaries().tobytes(), engine.segments_json(0), engine.snapshot_json(0), engine.text(0)))
    assert got[0] == got[1]
