"""What the critical document's ops do, from the CPU build of the row engine with event statistics
(tests/native MTE_CPU_STATS): per op, resolves and the rows they scan, heap pops and the heap size at
a pop, scour outcomes, packs, block splits and slots moved, and what a settle half on a second wave
would meet (handovers, first resolves that stand or are repeated). Sizes the device code paths (which path a
pop takes, how many rows a resolve sees). Usage: python tools/rg_stats.py [ops] [gid]"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import regcpu  # noqa: E402

NAMES = ["ops", "resolve", "res_rows", "res_nrows", "pop", "pop_big", "pop_heap", "find_rows", "scour", "scour_nop",
         "scour_serial", "scour_copy", "pack", "split_blk", "move_slots", "split_at", "zam_calls", "zam_pops", "lru_push",
         "range_rows", "duo_handover", "duo_spec_ok", "duo_spec_redo", "duo_no_resolve", "duo_w_rows",
         # removes: all; p2's block in p1's row; of those with no block split in the remove; rows the second
         # resolves scan (range_rows: rows the marking passes scan); pack's sibling pass: its scour calls and
         # the ones among them that left their block as it was
         "rem", "rem_same_row", "rem_same_row_no_blk_split", "res2_rows", "pack_scour", "pack_scour_nop",
         # a pack's shape: the sibling pass's second scour of the popped block changed it (not a no-op: a
         # tombstone the first pass dropped lets its neighbours join); the other siblings the pass changed;
         # packs with siblings in one row / two rows, with a sibling on the serial walk, with an arena_gc
         # during the pass, cascading into pack_internal, with 8 siblings (none: a level-1 node splits at
         # 8), ending with more blocks than siblings; the sums of siblings and of resulting blocks
         "pack_self_changed", "pack_sib_changed", "pack_one_row", "pack_two_rows", "pack_serial", "pack_gc",
         "pack_cascade", "pack_m8", "pack_grows", "pack_m_sum", "pack_kk_sum",
         # needsScour marks: as a second write of the row the edit has just written / folded into that write
         "lru_rewrite", "lru_folded",
         # packs the fused path took (pack_fused: all siblings decided at once, kept slots gathered by mask),
         # and the ones it handed back to the sibling loop: a sibling on the serial walk, an arena_gc needed
         "pack_fused", "pack_fused_fb_serial", "pack_fused_fb_gc",
         # the places round 13 restated (tests/test_reg_state_regs_cpu.py): resolves of documents of three or
         # more rows hitting in their first / second row buffer; block splits whose new block starts the next
         # row; heap entries written to register 1 / to registers 2..7; pops on the serial sift; packs by kk,
         # packs with T % kk != 0 (pack_internal's rounds count in both); pack_internal rounds; ops room() refused
         "hit_first", "hit_second", "split_next_row", "heap_reg1", "heap_reg2", "sift_serial", "pack_kk1", "pack_kk2",
         "pack_kk3", "pack_kk4", "pack_kk5", "pack_kk6", "pack_kk7", "pack_rem", "pack_internal", "room_refused"]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    gid = int(sys.argv[2]) if len(sys.argv) > 2 else 111877
    nat = os.path.join(ROOT, "tests", "native")
    subprocess.run(["make", "-s", "-C", nat, "stats"], check=True)
    L = ctypes.CDLL(os.path.join(nat, "_build", "libregcpu_stats.so"))
    regcpu._lib = None
    base = regcpu.lib()
    # the stats build exports the same entry points: route regcpu.replay through it
    L.regcpu_replay.restype = ctypes.c_uint64
    L.regcpu_replay.argtypes = base.regcpu_replay.argtypes
    L.regcpu_docres_size.restype = ctypes.c_uint32
    L.regcpu_heap.restype = ctypes.c_uint32
    L.regcpu_stats.restype = ctypes.c_uint32
    regcpu._lib = L
    ops, pay = regcpu.generated(2, gid, n, n_clients=8, seed=1000)
    at, res, rows, text = regcpu.replay(ops, pay)
    out = (ctypes.c_uint64 * 64)()
    L.regcpu_stats(out, len(NAMES) + 2)
    st = {k: int(out[i]) for i, k in enumerate(NAMES)}
    o = max(st["ops"], 1)
    per = {k: round(v / o, 4) for k, v in st.items() if k != "ops"}
    heap_max, lb_max = int(out[len(NAMES)]), int(out[len(NAMES) + 1])
    derived = {
        "rows_per_resolve": round(st["res_rows"] / max(st["resolve"], 1), 3),
        "nrows_at_resolve": round(st["res_nrows"] / max(st["resolve"], 1), 3),
        "heap_at_pop": round(st["pop_heap"] / max(st["pop"], 1), 1),
        "pops_on_serial_sift": round(st["pop_big"] / max(st["pop"], 1), 4),
        "slots_moved_per_split": round(st["move_slots"] / max(st["split_blk"] + st["pack"], 1), 1),
        "removes_same_row_share": round(st["rem_same_row"] / max(st["rem"], 1), 4),
        "removes_same_row_no_blk_split_share": round(st["rem_same_row_no_blk_split"] / max(st["rem"], 1), 4),
        "find_rows_per_pop": round(st["find_rows"] / max(st["pop"], 1), 3),
        "pack_scours_per_pack": round(st["pack_scour"] / max(st["pack"], 1), 3),
        "pack_siblings_changed_per_pack": round(st["pack_sib_changed"] / max(st["pack"], 1), 3),
        "pack_two_rows_share": round(st["pack_two_rows"] / max(st["pack"], 1), 4),
        "pack_serial_share": round(st["pack_serial"] / max(st["pack"], 1), 4),
        "pack_gc_share": round(st["pack_gc"] / max(st["pack"], 1), 6),
        "pack_cascade_share": round(st["pack_cascade"] / max(st["pack"], 1), 4),
        "pack_siblings_mean": round(st["pack_m_sum"] / max(st["pack"], 1), 3),
        "pack_blocks_out_mean": round(st["pack_kk_sum"] / max(st["pack"], 1), 3),
        # the fused pack: packs it took, and the share it handed back to the sibling loop
        "pack_fused_share": round(st["pack_fused"] / max(st["pack"], 1), 6),
        "pack_fused_fallback_share": round((st["pack_fused_fb_serial"] + st["pack_fused_fb_gc"]) / max(st["pack"], 1), 6),
        # a settle half on a second wave: of the ops after one whose settle pops, the
        # share whose first resolve would have to be repeated, and the rows a popping settle rewrites
        "duo_redo_share": round(st["duo_spec_redo"] / max(st["duo_spec_ok"] + st["duo_spec_redo"], 1), 4),
        "duo_rows_rewritten_per_handover": round(st["duo_w_rows"] / max(st["duo_handover"], 1), 3),
        "heap_max_at_pop": heap_max,
        "n_lb_max_at_pop": lb_max,
    }
    print(json.dumps({"doc": f"kind 2 gid {gid}, first {n} ops (CPU build of reg_engine.hpp)", "stop": int(at),
                      "max_lb": int(res["max_lb"]), "n_lb": int(res["n_lb"]), "height": int(res["height"]),
                      "heap_size_end": int(res["heap_size"]), "per_op": per, "derived": derived}, indent=1))


if __name__ == "__main__":
    main()
