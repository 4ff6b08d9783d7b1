"""Emission (emit.hip) at the sizes where its code paths change: rows of 32 / 33 units (one lane or
the whole wave sizes a row), surrogate pairs on the 64-unit steps of the whole-wave sizer and writer,
runs / joined pairs / elided rows on the 64-row batches of the walk, canAppend's 256, a run that ends
after a newline, chunk seams in both formats, property objects with array-index keys and at record
capacity, client names that need escaping -- and matchProperties on object values beyond the 64th of
a batch. Every document is built so that emission, not zamboni, meets the unmerged rows
(tests/emit_edges.py), and carries its own precondition, checked here on the oracle's JSON path
without a GPU; the GPU tests compare status, segment table and snapshot bytes with the oracle.
text() is not compared: it has no form for lone surrogates."""
import ctypes
import json

import pytest

from fluidframework_amd import mte
from oracle import OracleDoc
from tests import emit_edges as ee
from tests.gpu_helpers import dump, first_diff

CASES = ee.all_cases()
IDS = [c[0] for c in CASES]
MODES_SOLO = (3, 4)  # DocRes.mode: solo on the LDS engine / on the row engine


def records_equal_json(logs, chunk=10000):
    """The builder's record path = the JSON path (segment table and snapshot), per document."""
    b = mte.Builder()
    for log in logs:
        b.add_doc(json.dumps(log))  # ensure_ascii: lone surrogates travel as \\uXXXX
    batch = b.batch()
    for d, log in enumerate(logs):
        a, z = OracleDoc(), OracleDoc()
        a.apply_json(json.dumps(log))
        z.apply_batch(ctypes.addressof(batch), d)
        assert a.status()[0] == z.status()[0] == 0, (d, a.status(), z.status())
        assert a.segments_json() == z.segments_json(), d
        assert a.snapshot_json(chunk) == z.snapshot_json(chunk), d
    return batch


# ----------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name,log,check", CASES, ids=IDS)
def test_case_precondition(name, log, check, capsys):
    """The shape that makes the case meaningful, on the oracle's JSON path; the record path agrees."""
    assert len(log) <= 600
    said = check(ee.Shape(log))
    records_equal_json([log])
    with capsys.disabled():
        print(f"\n  {name}: {said}", end="")


def test_chunk_case_preconditions(capsys):
    """Case h: at chunks of 1 and 5 every document has a header and >= 3 body blobs, the exact-fit
    document >= 3 blobs at every size; the legacy header fills to the chunk and one body takes the rest."""
    said = []
    for name, log, _ in ee.chunk_cases():
        n = [len(ee.Shape(log, c).blobs) for c in ee.H_CHUNKS]
        assert min(n[:2]) >= 4 and (name != "h_exact" or min(n) >= 3), (name, n)  # >= 3 body blobs
        o = OracleDoc()
        o.apply_json(json.dumps(log))
        for c in ee.H_CHUNKS[:3] if name != "h_exact" else ee.H_CHUNKS:
            legacy = json.loads(o.snapshot_legacy_json(c))
            assert [e["path"] for e in legacy["entries"]][:2] == ["header", "body"], (name, c)
        said.append(f"{name}: {n} blobs at chunks {ee.H_CHUNKS}")
    with capsys.disabled():
        print("\n  " + "\n  ".join(said), end="")


def test_object_value_preconditions(capsys):
    logs, checks = ee.object_value_docs()
    said = [chk(ee.Shape(log)) for log, chk in zip(logs, checks) if chk]
    batch = records_equal_json(logs)
    vals = [ctypes.string_at(batch.val_text + batch.val_offsets[v], batch.val_offsets[v + 1] - batch.val_offsets[v])
            for v in range(batch.n_vals)]
    objs = [v for v in vals if v[:1] in (b"{", b"[")]
    assert len(objs) >= 70 and all(b'"n"' in v for v in objs[:70]), objs[:3]  # the pairs' values come after the 64th
    with capsys.disabled():
        print("\n  " + "\n  ".join(said) + f"\n  {len(objs)} object values in the batch, the pairs' after the 70th", end="")


# ----------------------------------------------------------------------------------------- GPU
def compare(engine, d, log, chunk=10000, legacy=False):
    """status, segment table, snapshot bytes of document d against the oracle's JSON path."""
    o = OracleDoc()
    o.apply_json(json.dumps(log))
    assert engine.status(d)[0] == o.status()[0] == 0, (d, engine.status(d), o.status())
    pairs = [("segments", engine.segments_json(d), o.segments_json())]
    if legacy:
        pairs.append(("legacy", engine.snapshot_legacy(d), o.snapshot_legacy_json(chunk)))
    else:
        pairs.append(("snapshot", engine.snapshot_json(d), o.snapshot_json(chunk)))
    for what, got, want in pairs:
        if got != want:
            dump(f"edges_doc{d}_{what}", got, want)
            i, ga, oa = first_diff(got, want)
            raise AssertionError(f"doc {d}: {what} differs at {i} (chunk {chunk})\n gpu: {ga}\n orc: {oa}")


def interleaved(cases):
    """The cases' logs with an empty document after every second one and at both ends."""
    logs = [[]]
    for i, c in enumerate(cases):
        logs.append(c[1])
        if i % 2:
            logs.append([])
    logs.append([])
    return logs


def run_batch(logs, chunk=10000, fmt=0):
    assert len(logs) < 100
    b = mte.Builder()
    for log in logs:
        b.add_doc(json.dumps(log))
    batch = b.batch()
    e = mte.Engine(0, chunk_size=chunk, snapshot_format=fmt)
    try:
        e.load(batch)
        st = e.replay()
        assert st["failed_docs"] == 0, st
        for d, log in enumerate(logs):
            compare(e, d, log, chunk, legacy=fmt == 1)
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_edge_cases_one_batch(order):
    """Every case in one batch beside empty documents, in the order given and reversed: a size
    miscounted in COUNT lands in a neighbour."""
    cases = CASES if order == "forward" else CASES[::-1]
    run_batch(interleaved(cases))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [0, 1], ids=["v1", "legacy"])
@pytest.mark.parametrize("chunk", ee.H_CHUNKS)
def test_chunk_seams(chunk, fmt):
    """Case h: COUNT and WRITE agree on where a chunk closes; the legacy header fills to the chunk."""
    run_batch(interleaved(ee.chunk_cases()), chunk, fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [7, 8])
def test_map_record_capacity(n):
    """A batch whose widest map has 7 keys takes the narrow map record and fills it; 8 keys the wide one."""
    name, log, check = ee.case_i_map(n)
    check(ee.Shape(log))
    run_batch([[], log, ee.case_a("ascii")[1]])


@pytest.mark.gpu
def test_second_emission_round():
    """Solo documents are emitted in round 1, after the pass: one document each of b, d and f alone."""
    e = mte.Engine(0)
    try:
        e.set_option("solo_min_ops", 1)
        for name in ("bc_end_hi", "d_63_pair", "f_63_40"):
            log = CASES[IDS.index(name)][1]
            b = mte.Builder()
            b.add_doc(json.dumps(log))
            e.load(b.batch())
            e.replay()
            r = e.doc_result(0)
            assert e.run_info()["solo"] == 1 and r["mode"] in MODES_SOLO, (name, r, e.run_info())
            compare(e, 0, log)
    finally:
        e.close()


@pytest.mark.gpu
def test_object_values_beyond_64():
    """matchProperties on object values (properties.ts:72-80) interned after 70 distinct ones: key
    order and array / index-object forms are equal, so the rows merge (zamboni) or coalesce
    (emission) as on the oracle; the control pair stays apart."""
    logs, checks = ee.object_value_docs()
    for log, chk in zip(logs, checks):
        if chk:
            chk(ee.Shape(log))
    run_batch(logs)
    run_batch(logs, fmt=1)


def test_object_value_limit_precondition():
    """32 and 33 pairs of rows whose object values are equal in another key order (64 and 66 values
    that each equal another value of the batch): every pair is one entry on the oracle."""
    for pairs in (32, 33):
        log = ee.object_limit_log(pairs)
        records_equal_json([log])
        txt = [ee.Shape.entry_text(x) for x in ee.Shape(log).entries]
        assert all(f"p{i:02d}q{i:02d}" in txt for i in range(pairs)), txt


@pytest.mark.gpu
def test_object_value_limit_on_gpu():
    """The match table has 64 columns, one per object value that equals another value of the batch:
    64 such values load and match the oracle, 66 are a load error, never a different result."""
    run_batch([ee.object_limit_log(32)])
    b = mte.Builder()
    b.add_doc(json.dumps(ee.object_limit_log(33)))
    e = mte.Engine(0)
    try:
        with pytest.raises(mte.MteError, match="object values"):
            e.load(b.batch())
    finally:
        e.close()
