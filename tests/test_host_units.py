"""The layout of the host units in fluidframework_amd/csrc (source text only, no GPU needed): which
unit may call HIP or see RCCL, and that the Makefile links every unit."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluidframework_amd", "csrc")

HIP_CALL = re.compile(r"\bhip[A-Z]\w*\s*\(")


def read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def units():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.cpp")))


def test_hip_free_units_and_rccl_include():
    # the read-back and the builder reach the device through engine_host.hpp's functions only
    for name in ("readback.cpp", "builder.cpp"):
        calls = HIP_CALL.findall(read(name))
        assert not calls, f"{name} calls the HIP API: {sorted(set(calls))}"
    # the planning half of incremental replay stands without the engine object (tests/native/ck_plan_main.cpp)
    calls = HIP_CALL.findall(read("ck_plan.hpp"))
    assert not calls, f"ck_plan.hpp calls the HIP API: {sorted(set(calls))}"
    assert not re.search(r"#\s*include\s*\"engine_host\.hpp\"", read("ck_plan.hpp"))
    sources = units() + sorted(
        os.path.basename(p) for ext in ("*.hpp", "*.h", "*.hip") for p in glob.glob(os.path.join(CSRC, ext))
    )
    with_rccl = [n for n in sources if re.search(r"#\s*include\s*<rccl/rccl\.h>", read(n))]
    assert with_rccl == ["gather.cpp"]


def test_makefile_links_every_unit():
    assert not os.path.exists(os.path.join(CSRC, "mte_host.cpp"))
    names = units()
    assert {"engine_load.cpp", "engine_run.cpp", "engine_ckpt.cpp", "readback.cpp", "gather.cpp", "diag.cpp", "builder.cpp"} <= set(names)
    makefile = read("Makefile").replace("\\\n", " ")
    m = re.search(r"^OBJS\s*:=\s*(.*)$", makefile, re.M)
    assert m, "the Makefile defines no OBJS"
    objs = set(re.findall(r"/(\w+)\.o\b", m.group(1)))
    missing = [n for n in names if n[:-4] not in objs]
    assert not missing, f"not in the Makefile's OBJS: {missing}"
