"""The marker queries without a GPU: the Python restatement the GPU tests compare against
(tests/markers.py) on the reference's own spec cases -- the eight findTile cases of client.spec.ts:28-233 and
the getTextAndMarkers case of sharedString.spec.ts:150-182, restated as one-writer observer logs, with the
spec's literal positions -- the tag table hand-derived from textSegment.ts:196-240, the shapes the GPU
tests' logs rely on, and the host plan and the CPU build of the wave programs as a stand-alone program under
ASan and UBSan."""
import os
import subprocess

import pytest

from oracle import OracleDoc
from tests import markers
from tests.markers import OBSERVER, Writer, find_tile, paragraphs, tile
from tests.oplog import dumps
from tests.views import rows_of, units

_NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
_PROG = os.path.join(_NATIVE, "_build", "marker_main")
EOP = tile(("EOP",), markerId="some-id")


def table(log):
    o = OracleDoc(OBSERVER)
    o.apply_json(dumps(log))
    assert o.status()[0] == 0, o.status()
    return rows_of(o)


def pos_of(t):
    return None if t is None else t[1]


def spec_doc(steps):
    """insertMarkerLocal / insertTextLocal calls as one writer's log."""
    w = Writer()
    for pos, seg in steps:
        w.insert(pos, seg)
    return table(w.log), w.length


def test_find_non_preceding_tile_by_label():  # client.spec.ts:29-51
    rows, length = spec_doc([(0, EOP), (0, "abc")])
    assert length == 4
    assert pos_of(find_tile(rows, 0, "EOP", False)) == 3


def test_find_non_preceding_tile_single_tile():  # :53-73
    rows, length = spec_doc([(0, "abc d"), (0, EOP)])
    assert length == 6
    assert pos_of(find_tile(rows, 0, "EOP", False)) == 0


MULTI = [(0, EOP), (0, "abc d"), (0, EOP), (7, "ef"), (8, EOP)]


def test_find_preceding_tile_multiple_tiles():  # :75-112
    rows, length = spec_doc(MULTI)
    assert length == 10
    assert pos_of(find_tile(rows, 5, "EOP")) == 0


def test_find_non_preceding_tile_multiple_tiles():  # :114-151
    rows, length = spec_doc(MULTI)
    assert pos_of(find_tile(rows, 5, "EOP", False)) == 6


def test_find_tile_length_one():  # :153-178
    rows, length = spec_doc([(0, EOP)])
    assert length == 1
    assert pos_of(find_tile(rows, 0, "EOP")) == 0
    assert pos_of(find_tile(rows, 0, "EOP", False)) == 0


def test_index_out_of_bound():  # :180-204
    rows, length = spec_doc([(0, EOP), (0, "abc")])
    assert length == 4
    assert pos_of(find_tile(rows, 5, "EOP")) == 3
    assert find_tile(rows, 5, "EOP", False) is None


def test_text_without_the_tile():  # :206-220
    rows, length = spec_doc([(0, "abc")])
    assert length == 3
    assert find_tile(rows, 1, "EOP") is None and find_tile(rows, 1, "EOP", False) is None


def test_null_text():  # :222-232
    rows, _ = spec_doc([])
    assert find_tile(rows, 1, "EOP") is None and find_tile(rows, 1, "EOP", False) is None


def test_shared_string_get_text_and_markers():  # sharedString.spec.ts:150-182
    w = Writer()
    w.insert(0, "hello world")
    w.insert(6, {"marker": {"refType": 0}, "props": {"markerId": "markerId", "markerSimpleType": "markerKeyValue"}})
    w.insert(0, tile(("tileLabel",), markerId="tileMarkerId"))
    rows = table(w.log)
    got = paragraphs(rows, "tileLabel")
    assert len(got) == 1 and got[0]["pos"] == 0 and got[0]["units"] == []
    assert markers.props_of(rows[got[0]["row"]])["markerId"] == "tileMarkerId"
    assert paragraphs(rows, "other") == []


# textSegment.ts:196-240 by hand. tagsInProgress P, the row's tag list T -> (endTags + beginTags, P after):
# T non-empty: <t> for t of T not in P; </p> for p of P not in T; the new tags pushed in reverse; the closed ones
# removed. T empty: every p of P closed in P's order.
TAG_TABLE = {
    ("", ""): ("", ""), ("", "b"): ("<b>", "b"), ("", "u"): ("<u>", "u"), ("", "bu"): ("<b><u>", "ub"),
    ("b", ""): ("</b>", ""), ("b", "b"): ("", "b"), ("b", "u"): ("</b><u>", "u"), ("b", "bu"): ("<u>", "bu"),
    ("u", ""): ("</u>", ""), ("u", "b"): ("</u><b>", "b"), ("u", "u"): ("", "u"), ("u", "bu"): ("<b>", "ub"),
    ("ub", ""): ("</u></b>", ""), ("ub", "b"): ("</u>", "b"), ("ub", "u"): ("</b>", "u"), ("ub", "bu"): ("", "ub"),
    ("bu", ""): ("</b></u>", ""), ("bu", "b"): ("</u>", "b"), ("bu", "u"): ("</b>", "u"), ("bu", "bu"): ("", "bu"),
}


@pytest.mark.parametrize("state,tags", sorted(TAG_TABLE))
def test_tag_table(state, tags):
    in_progress = list(state)
    props = {"font-weight": "bold" if "b" in tags else None, "text-decoration": "underline" if "u" in tags else 0}
    out = markers.gather_tags(props, in_progress)
    assert (out, "".join(in_progress)) == TAG_TABLE[state, tags]


def test_tag_states_are_closed():
    """The five states are all the table reaches from [], and it reaches every one of them."""
    seen, todo = {""}, [""]
    while todo:
        s = todo.pop()
        for t in ("", "b", "u", "bu"):
            n = TAG_TABLE[s, t][1]
            if n not in seen:
                seen.add(n)
                todo.append(n)
    assert seen == {"", "b", "u", "ub", "bu"}


def test_tags_through_a_document():
    """[b] meeting [b, u] becomes [b, u], and a later close prints </b></u>; the state crosses a tile."""
    w = Writer()
    w.append(markers.text_seg("a", bold="bold"))
    w.append(markers.text_seg("b", bold="bold", under="underline"))
    w.append(tile())
    w.append("c")
    w.append(tile())
    w.append("dropped")
    got = paragraphs(table(w.log), "EOP")
    assert [(p["pos"], bytes(p["units"]).decode()) for p in got] == [(2, "<b>a<u>b"), (4, "</b></u>c")]


def test_seam_log_shape():
    log = markers.seam_log()
    rows = table(log)
    assert len(rows) == 140
    assert [i for i, r in enumerate(rows) if r["kind"] == "M"] == [0, 62, 63, 64, 65, 139]
    # a BEFORE whose answer lies two steps back, an AFTER whose answer lies two steps ahead
    assert find_tile(rows, 2 * 131, "EOP")[0] == 65 and find_tile(rows, 1, "EOP", False)[0] == 62
    far = table(markers.seam_log(200, tiles=(0,)))
    assert find_tile(far, 380, "EOP") == (0, 0) and find_tile(far, 5, "EOP", False)[0] == 199


def test_removed_last_tile_is_found_at_the_length():
    w = Writer()
    w.append("ab")
    w.append(tile())
    w.remove(2, 3, client="r")
    rows = table(w.log)
    assert len(rows) == 2 and "removedSeq" in rows[1]
    assert find_tile(rows, 2, "EOP", False) == (1, 2) and find_tile(rows, 1, "EOP", False) is None
    assert find_tile(rows, 2, "EOP") is None and find_tile(rows, 3, "EOP", False) is None


def test_label_values():
    w = Writer()
    for v in (("EOP",), ("H1", "EOP", "Q"), "EOP", "xEy", None, 7, True, {"EOP": 1}):
        w.append(tile(v))
    w.append(tile(("EOP",), ref_type=2))  # the label without the Tile bit
    rows = table(w.log)
    assert [markers.has_tile_label(r, "EOP") for r in rows] == [True, True, False, False, False, False, False, False, False]
    assert [markers.has_tile_label(r, "E") for r in rows] == [False, False, True, True, False, False, False, False, False]
    assert units("\U0001F600") == [0xD83D, 0xDE00]


def test_marker_plan_and_wave_programs_standalone():
    subprocess.run(["make", "-s", "-C", _NATIVE, "-f", "marker.mk", "_build/marker_main"], check=True)
    needed = subprocess.run(["ldd", _PROG], check=True, capture_output=True, text=True).stdout
    assert "amdhip" not in needed and "libmte" not in needed, needed
    r = subprocess.run([_PROG], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]  # no failed check, no sanitizer report
    assert r.stdout.startswith("ok: "), r.stdout
