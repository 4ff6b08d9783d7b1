"""GPU: the row engine's critical-path shortcuts (reg_engine.hpp: the heap pop fused with the popped
segment's search, the lane-parallel sift path) on every device instantiation -- k_solo lean, PROPS + WIDE (FULL), and k_rows at 4 and 12
waves -- against the oracle: status, text, segment table and SnapshotV1 bytes (tests/gpu_helpers.py).
The shapes are the smallest at which a second row, a block split inside a remove, a pack with siblings
in two rows and a heap of more than 64 entries all occur (3 000 kind-2 ops: heap 65+ at a pop, checked
on the CPU build by tests/test_reg_scan_diet_cpu.py::test_gpu_case_heap_passes_64_entries)."""
import pytest

from fluidframework_amd import mte
from tests.gpu_helpers import compare_batch_checksums, compare_doc

pytestmark = pytest.mark.gpu

MODE_ROWS, MODE_BULK_ROWS = 4, 5


@pytest.fixture(scope="module")
def engine():
    e = mte.Engine(0)
    e.set_option("solo_min_ops", 1)  # one-document batches take the solo route
    yield e
    e.set_option("rows_bulk", -1)
    e.close()


@pytest.mark.parametrize("kind,n_ops,clients,gid,lean", [(2, 3000, 8, 1, 1), (3, 2000, 8, 7, 0), (2, 1200, 33, 3, 0),
                                                         (3, 1100, 33, 2, 0)])
def test_lone_document_on_k_solo(engine, kind, n_ops, clients, gid, lean):
    """One document on k_solo: lean (kind 2), PROPS + WIDE with properties (kind 3: ties, overlapping
    removes, annotates), and 33 writers (removers past 32)."""
    engine.set_option("rows_bulk", -1)
    engine.generate(kind, 1, n_ops, n_clients=clients, seed=17 if lean else 1000, doc_ids=[gid])
    batch = engine.export_batch()
    st = engine.replay()
    info = engine.run_info()
    assert info["solo"] == 1 and info["lean"] == lean, info
    r = engine.doc_result(0)
    assert r["status"] == 0 and st["ops"] == n_ops and r["mode"] == MODE_ROWS, r
    if lean:
        assert r["max_lb"] > 8, r  # a second row
    compare_doc(engine, batch, 0)


@pytest.mark.parametrize("waves", [4, 12])
@pytest.mark.parametrize("kind,n_ops,clients", [(2, 3000, 8), (3, 2000, 8), (2, 300, 33)])
def test_documents_on_k_rows(engine, kind, n_ops, clients, waves):
    """The same shapes as bulk documents on k_rows (fixed quarters at 4 waves, the paged pool at 12):
    every checksum against the oracle, the first documents in full."""
    engine.set_option("rows_bulk", waves)
    try:
        engine.generate(kind, 48, n_ops, n_clients=clients, seed=1000)
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
