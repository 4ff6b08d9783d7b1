"""The host arithmetic of incremental replay (option retain) without a GPU: fluidframework_amd/csrc/ck_plan.hpp
-- the prefix check that offers a checkpoint, the id translation when a fresh builder numbers keys and
values in another order, the regions of a pass and the block documents' admission to the budget --
driven by tests/native/ck_plan_main.cpp on batches of the real builder (builder.cpp). A stand-alone host
program under AddressSanitizer and UBSan, linked without the HIP runtime and without libmte.so; the
cases and their expected values are in the program."""
import os
import subprocess

_NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
_PROG = os.path.join(_NATIVE, "_build", "ck_plan_main")


def test_ck_plan_standalone():
    subprocess.run(["make", "-s", "-C", _NATIVE, "_build/ck_plan_main"], check=True)
    needed = subprocess.run(["ldd", _PROG], check=True, capture_output=True, text=True).stdout
    assert "amdhip" not in needed and "libmte" not in needed, needed
    r = subprocess.run([_PROG], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]  # no failed check, no sanitizer report
    assert r.stdout.startswith("ok: "), r.stdout
