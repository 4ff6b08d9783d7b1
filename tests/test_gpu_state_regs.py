"""GPU: the row engine after round 13 (reg_engine.hpp: heap entries written in place by lane compare and
the pack's division by a multiplier, on lean k_solo) on every device instantiation -- k_solo
lean, PROPS + WIDE and 33 writers (which keep the code they had), a lean document that hands over to the LDS
engine between two ops with a heap past 127 entries, and k_rows at 4 and 12 waves, which must be the
kernels they were -- against the oracle: status, text, segment table and SnapshotV1 bytes
(tests/gpu_helpers.py). The k_solo documents are those of tests/state_regs_docs.py;
tests/test_reg_state_regs_cpu.py asserts on the CPU build which places of the engine they reach."""
import pytest

from fluidframework_amd import mte
from tests.gpu_helpers import compare_batch_checksums, compare_doc
from tests.state_regs_docs import FULL, HANDOFF, LEAN, W33

pytestmark = pytest.mark.gpu

MODE_SOLO_LDS, MODE_ROWS, MODE_BULK_ROWS = 3, 4, 5


@pytest.fixture(scope="module")
def engine():
    e = mte.Engine(0)
    e.set_option("solo_min_ops", 1)  # one-document batches take the solo route
    yield e
    e.set_option("rows_bulk", -1)
    e.close()


@pytest.mark.parametrize("doc,lean,mode", [(LEAN, 1, MODE_ROWS), (FULL, 0, MODE_ROWS), (W33, 0, MODE_ROWS),
                                           (HANDOFF, 1, MODE_SOLO_LDS)],
                         ids=["lean", "props_wide", "33_writers", "handoff"])
def test_lone_document_on_k_solo(engine, doc, lean, mode):
    """One document on k_solo. The handoff document (31 writers) outgrows the row plan at op 1255 and must
    finish on the LDS engine with the oracle's result."""
    kind, gid, n_ops, clients, seed = doc
    engine.set_option("rows_bulk", -1)
    engine.generate(kind, 1, n_ops, n_clients=clients, seed=seed, doc_ids=[gid])
    batch = engine.export_batch()
    st = engine.replay()
    info = engine.run_info()
    assert info["solo"] == 1 and info["lean"] == lean, info
    r = engine.doc_result(0)
    assert r["status"] == 0 and st["ops"] == n_ops and r["mode"] == mode, r
    if doc is LEAN:
        assert r["max_lb"] > 16, r  # three rows and more
    compare_doc(engine, batch, 0)


@pytest.mark.parametrize("waves", [4, 12])
@pytest.mark.parametrize("kind,n_ops", [(2, 3000), (3, 2000), (5, 2000)])
def test_documents_on_k_rows(engine, kind, n_ops, waves):
    """48 bulk documents on k_rows (fixed quarters at 4 waves, the paged pool at 12): every checksum
    against the oracle, the first documents in full."""
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
