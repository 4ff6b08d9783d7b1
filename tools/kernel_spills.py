"""Register and spill counts of the row-engine kernels (k_solo / k_rows / k_rows_cont) of one or more
libmte.so builds, from the metadata notes of the gfx950 code objects bundled in each library.
Usage: python tools/kernel_spills.py [name=]path/to/libmte.so ...   -> one JSON object per library
(needs llvm-readelf from the ROCm LLVM tools; uncompressed offload bundles)."""
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
READELF = os.environ.get("READELF", "/opt/rocm/llvm/bin/llvm-readelf")
KEYS = ("sgpr_count", "vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")


def code_objects(blob):
    at = 0
    while True:
        at = blob.find(MAGIC, at)
        if at < 0:
            return
        n = struct.unpack_from("<Q", blob, at + len(MAGIC))[0]
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24: p + 24 + tl].decode()
            p += 24 + tl
            if "gfx" in triple and size:
                yield blob[at + off: at + off + size]
        at = p


def kernels(path):
    out = {}
    blob = open(path, "rb").read()
    for co in code_objects(blob):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name:
                continue
            vals = {k: int(m.group(1)) for k in KEYS if (m := re.search(r"\.%s:\s+(\d+)" % k, blk))}
            out[name.group(1)] = vals
    names = list(out)
    cxxfilt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")  # mangled names stay without one
    if names and cxxfilt:
        dem = subprocess.run([cxxfilt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        out = {d.split("(")[0]: out[n] for n, d in zip(names, dem)}
    return {k: v for k, v in sorted(out.items()) if re.search(r"k_solo|k_rows", k)}


def main():
    for a in sys.argv[1:]:
        name, _, path = a.rpartition("=")
        print(json.dumps({"lib": name or path, "kernels": kernels(path)}, indent=1))


if __name__ == "__main__":
    main()
