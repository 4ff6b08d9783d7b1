"""Register copies in the row-engine kernels' assembly: instructions that move a value and compute nothing.
Per kernel of an assembly file (`make asm-solo`: mte_solo.hip with the library's flags) it reports
  instructions / valu        all instructions, and the vector-ALU ones among them
  mov_b32 / mov_b64          plain vector register-to-register moves (v_mov_b32 vN, vM; v_mov_b64 v[..], v[..])
  spill_writelane / spill_readlane
                             immediate-lane v_writelane / v_readlane on the VGPRs that hold spilled SGPRs
                             (spill_vgprs: registers written by immediate-lane v_writelane and nothing else)
  batches                    runs of 6 or more consecutive copies: {size: how many}, and the registers they move
  divisions                  float-reciprocal integer divisions (one v_rcp_iflag_f32 each)
With an MTE_MARKERS build (make asm-solo EXTRA=-DMTE_MARKERS) --scopes adds the same figures per RG_PROF
scope, exclusive of nested scopes, as tools/asm_regions.py does for instructions.
Usage: python tools/asm_copies.py fluidframework_amd/_build/mte_solo.s [--kernel SUBSTR] [--scopes] [--batches]
(--kernel matches the demangled name, e.g. 'k_solo<false, 0, false>'; --batches lists every batch's line)
It counts ordinary moves only, and prints one JSON object."""
import argparse
import json
import re
import shutil
import subprocess
from collections import Counter

# row-engine scopes (reg_engine.hpp RgProf; markers are 100 + slot)
RG_NAMES = ["total", "fetch", "apply", "resolve", "insert_slot", "split", "range", "zamboni", "scour", "heap", "find_seg",
            "pack", "lru", "ops", "n_resolve", "n_scour", "n_scour_changed", "n_pack", "n_pop", "n_split_blk", "n_move",
            "split_at", "ins", "rem", "msn", "zam_edit", "pack_sibs", "pack_fused"]


def scope_name(s):
    return RG_NAMES[s - 100] if 100 <= s < 100 + len(RG_NAMES) else str(s)


INS = re.compile(r"^\s+((?:[sv]|ds|global|scratch|buffer|flat)_[a-z0-9_]+)\s*(.*?)\s*(?:;.*)?$")
VREG = r"v\d+"
VPAIR = r"v\[\d+:\d+\]"
MOV32 = re.compile(r"^v_mov_b32(?:_e32|_e64)?$")
MOV64 = re.compile(r"^v_mov_b64(?:_e32|_e64)?$")
WLANE = re.compile(r"^v_writelane_b32$")
RLANE = re.compile(r"^v_readlane_b32$")
IMM = re.compile(r"^(?:\d+|0x[0-9a-fA-F]+)$")
BATCH_MIN = 6


def functions(lines):
    """(name, first line, last line) of every function: from its label to its .Lfunc_end"""
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if m:
            j = i + 1
            while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
                j += 1
            yield m.group(1), i + 1, j
            i = j
        i += 1


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return {n: d.split("(")[0].replace("void ", "") for n, d in zip(names, out)}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def classify(mn, ops):
    """'b32' / 'b64' for a vector register-to-register move, 'wl' / 'rl' for an immediate-lane lane move, else None"""
    a = [x.strip() for x in ops.split(",")]
    if MOV32.match(mn) and len(a) == 2 and re.fullmatch(VREG, a[0]) and re.fullmatch(VREG, a[1]):
        return "b32"
    if MOV64.match(mn) and len(a) == 2 and re.fullmatch(VPAIR, a[0]) and re.fullmatch(VPAIR, a[1]):
        return "b64"
    if WLANE.match(mn) and len(a) == 3 and IMM.match(a[2]):
        return "wl"
    if RLANE.match(mn) and len(a) == 3 and IMM.match(a[2]):
        return "rl"
    return None


def new_counts():
    return {"instructions": 0, "valu": 0, "mov_b32": 0, "mov_b64": 0, "spill_writelane": 0, "spill_readlane": 0,
            "divisions": 0, "batches": Counter(), "batch_copies": 0, "batch_regs": 0}


def analyse(lines, lo, hi, scopes, list_batches):
    # pass 1: the VGPRs that hold spilled SGPRs: written by immediate-lane v_writelane, by nothing else
    lane_w, other_w = Counter(), set()
    parsed = []
    for n in range(lo, hi):
        m = INS.match(lines[n])
        if not m:
            parsed.append(None)
            continue
        mn, ops = m.group(1), m.group(2)
        kind = classify(mn, ops)
        parsed.append((mn, ops, kind))
        dst = ops.split(",")[0].strip()
        if kind == "wl":
            lane_w[dst] += 1
        elif mn.startswith("v_") or mn.startswith(("ds_", "global_", "scratch_", "buffer_", "flat_")):
            r = re.fullmatch(r"v\[(\d+):(\d+)\]", dst)
            if r:
                other_w.update("v%d" % x for x in range(int(r.group(1)), int(r.group(2)) + 1))
            elif re.fullmatch(VREG, dst):
                other_w.add(dst)
    spill = {v for v in lane_w if v not in other_w}
    # pass 2: the counts, for the kernel and per scope (exclusive)
    tot = new_counts()
    per = {}
    stack = []
    run, run_regs, run_at = 0, 0, 0
    found = []

    def close(where):
        nonlocal run, run_regs
        if run >= BATCH_MIN:
            for c in where:
                c["batches"][run] += 1
                c["batch_copies"] += run
                c["batch_regs"] += run_regs
            if list_batches:
                found.append({"line": run_at + 1, "copies": run, "regs": run_regs,
                              "scope": scope_name(stack[-1]) if stack else None})
        run = run_regs = 0

    for off, pr in enumerate(parsed):
        line = lines[lo + off]
        here = [tot] + ([per.setdefault(stack[-1], new_counts())] if scopes and stack else [])
        if pr is None:
            b = re.search(r"MTE_BEGIN (0x[0-9a-fA-F]+|\d+)", line)
            e = re.search(r"MTE_END (0x[0-9a-fA-F]+|\d+)", line)
            if b or e or re.match(r"^\.?\w+:", line):  # a scope edge or a label ends a batch
                close(here)
            if b:
                stack.append(int(b.group(1), 0))
            elif e and stack and stack[-1] == int(e.group(1), 0):
                stack.pop()
            continue
        mn, ops, kind = pr
        a = [x.strip() for x in ops.split(",")]
        if kind == "wl" and a[0] not in spill:
            kind = None
        if kind == "rl" and a[1] not in spill:
            kind = None
        for c in here:
            c["instructions"] += 1
            c["valu"] += mn.startswith("v_")
            c["divisions"] += mn.startswith("v_rcp_iflag_f32")
            if kind == "b32":
                c["mov_b32"] += 1
            elif kind == "b64":
                c["mov_b64"] += 1
            elif kind == "wl":
                c["spill_writelane"] += 1
            elif kind == "rl":
                c["spill_readlane"] += 1
        if kind in ("b32", "b64"):
            if not run:
                run_at = lo + off
            run += 1
            run_regs += 2 if kind == "b64" else 1
        else:
            close(here)
    close([tot])

    def fin(c):
        c = dict(c)
        c["batches"] = {str(k): v for k, v in sorted(c["batches"].items())}
        return c

    out = fin(tot)
    out["spill_vgprs"] = sorted(spill, key=lambda v: int(v[1:]))
    if scopes:
        out["scopes"] = {scope_name(s): fin(c) for s, c in sorted(per.items())}
    if list_batches:
        out["batch_list"] = found
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("--kernel", default="k_", help="substring of the demangled kernel name (default: every k_* kernel)")
    ap.add_argument("--scopes", action="store_true", help="per RG_PROF scope (MTE_MARKERS build)")
    ap.add_argument("--batches", action="store_true", help="list every batch with its line")
    a = ap.parse_args()
    lines = open(a.asm).read().split("\n")
    fns = list(functions(lines))
    dem = demangle([f[0] for f in fns])
    out = {}
    for nm, lo, hi in fns:
        if a.kernel in dem[nm]:
            out[dem[nm]] = analyse(lines, lo, hi, a.scopes, a.batches)
    print(json.dumps({"asm": a.asm, "kernels": out}, indent=1))


if __name__ == "__main__":
    main()
