"""The view queries without a GPU: the Python restatement the GPU tests compare against (tests/views.py)
is itself pinned to the oracle -- its view length to OracleDoc.length_at for every client, and its text
to a fresh oracle fed only a prefix of the log (which does not depend on the predicate's remove branch
being right by construction) -- the logs of the GPU tests have the shapes those tests rely on, and the
host plan and the CPU build of the wave programs run as a stand-alone program under ASan and UBSan."""
import os
import subprocess

import pytest

from oracle import OracleDoc
from tests import views
from tests.oplog import dumps
from tests.test_gpu_fuzz import random_json_log
from tests.test_many_clients import overlap_log

WRITERS = [2, 3, 8, 20, 40, 70]
_NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
_PROG = os.path.join(_NATIVE, "_build", "view_main")


def replayed(log, observer=views.OBSERVER):
    o = OracleDoc(observer)
    o.apply_json(dumps(log))
    assert o.status()[0] == 0, o.status()
    return o


def short_ids(log):
    order = []
    for m in log:
        if m["clientId"] not in order:
            order.append(m["clientId"])
    return {c: i + 1 for i, c in enumerate(order)}


@pytest.mark.parametrize("seed", range(12))
def test_view_length_matches_oracle_length_at(seed):
    log = views.no_msn(random_json_log(seed, 400, n_writers=WRITERS[seed % 6], emoji=False))
    o = replayed(log)
    rows = views.rows_of(o)
    ids = dict(short_ids(log), **{views.OBSERVER: 0})
    n = 0
    for ref in range(0, len(log) + 1, 7):
        for name, short in ids.items():
            assert views.length(rows, ref, name) == o.length_at(ref, short), (seed, ref, name)
            n += 1
    assert n > 100 and len(rows) > 300


@pytest.mark.parametrize("seed", range(12))
def test_prefix_identity(seed):
    """No client's view at ref_seq r is the document after the messages up to r."""
    log = views.no_msn(random_json_log(seed, 400, n_writers=WRITERS[seed % 6], emoji=False))
    rows = views.rows_of(replayed(log))
    for r in range(0, len(log) + 1, 25):
        want = replayed([m for m in log if m["sequenceNumber"] <= r]).text()
        assert views.text(rows, r, None) == views.units(want), (seed, r)


def test_seam_logs_have_the_row_counts():
    for n in views.SEAM_SIZES:
        log = views.seam_log(n)
        rows = views.rows_of(replayed(log))
        assert len(rows) == n
        for i, who in views.SEAM_REMOVERS.items():
            if i < n:
                assert rows[i]["removedClient"] == who
        assert sum("removedSeq" in r for r in rows) == sum(i < n for i in views.SEAM_REMOVERS)
        # rows of length 0 on both sides of every 64-row step the document has, in the newest view; an
        # older view still counts some of them
        gone = [i for i in views.SEAM_REMOVERS if i < n]
        lens = [views.view_len(r, len(log), None) for r in rows]
        assert [i for i, v in enumerate(lens) if v == 0] == gone
        if len(gone) > 1:
            older = [views.view_len(r, len(log) - 1, None) for r in rows]
            assert [i for i, v in enumerate(older) if v == 0] == gone[1:]


def test_overlap_log_uses_the_second_overlap_word():
    log = overlap_log(100)
    rows = views.rows_of(replayed(log))
    ids = short_ids(log)
    seen = {ids[c] for r in rows for c in r["overlap"]}
    for s in (31, 32, 63, 64, 65, 100):
        assert s in seen, s


def test_view_plan_and_wave_programs_standalone():
    subprocess.run(["make", "-s", "-C", _NATIVE, "-f", "view.mk", "_build/view_main"], check=True)
    needed = subprocess.run(["ldd", _PROG], check=True, capture_output=True, text=True).stdout
    assert "amdhip" not in needed and "libmte" not in needed, needed
    r = subprocess.run([_PROG], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]  # no failed check, no sanitizer report
    assert r.stdout.startswith("ok: "), r.stdout
