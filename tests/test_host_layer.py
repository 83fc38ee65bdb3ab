"""CPU checks of the host layer the C-ABI libraries share (humanoid_amd/csrc/he_host.h): the owning
device arrays and the query libraries' create, destroy and call checks under a host sanitizer, as a
stand-alone program against a counting allocator (tests/host/device_array_test.cpp), and the error
text, which each library keeps for itself."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "humanoid_amd", "csrc")


def _rocm_include():
    from humanoid_amd import build
    hipcc = shutil.which(build._hipcc()) or build._hipcc()
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    assert os.path.exists(os.path.join(inc, "hip", "hip_runtime_api.h")), inc
    return inc


def test_device_arrays_own_their_memory_under_a_sanitizer(tmp_path):
    """he_host.h builds with the plain host compiler, and its arrays free what they hold exactly once on
    every path: a failed k-th allocation of a sequence, move assignment, the staged replace of the motion
    tables with any step failing, a zero-length array. The query libraries' shared create and destroy,
    with a toy handle and model: every argument refusal leaves the output null and allocates nothing, a
    failed allocation or copy leaves nothing alive, a created handle is freed once, destroying null is 0;
    and the refusals their calls share, text by text. AddressSanitizer (with its leak check) and UBSan
    watch the run; the program's own counters are asserted in it."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "device_array_test"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", _rocm_include(), "-I", CSRC,
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "device_array_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "he_host ownership: ok" in r.stdout


def test_host_header_is_host_only():
    """No device code in the header, and nothing included but the HIP runtime API and the standard library."""
    import re
    text = open(os.path.join(CSRC, "he_host.h")).read()
    assert not re.search(r"__(device|global|shared)__", text)
    incs = re.findall(r"#include\s+(\S+)", text)
    assert "<hip/hip_runtime_api.h>" in incs
    assert all(i.startswith("<") and (i == "<hip/hip_runtime_api.h>" or "/" not in i and "." not in i) for i in incs), incs


def test_each_library_keeps_its_own_error_text(he_model):
    """All four libraries in one process: an argument error in each leaves the others' text alone."""
    from humanoid_amd import build, dynamics, engine, render, solve
    if not all(os.path.exists(p) for p in (engine.LIB_PATH, render.LIB_PATH, dynamics.LIB_PATH, solve.LIB_PATH)):
        build.build()
    he, hr, hd, hs = engine.load_library(), render.load_library(), dynamics.load_library(), solve.load_library()
    assert hd.hd_compute(None, None, None, None, None, None, 1, None) != 0
    assert hr.hr_render(None, None, None, None, None, 3, None) != 0
    assert he.he_create(None, 0, None) != 0
    texts = [f().decode() for f in (hd.hd_last_error, hr.hr_last_error, he.he_last_error)]
    assert texts[0].startswith("hd_compute: null handle"), texts
    assert texts[1].startswith("hr_render: null handle"), texts
    assert texts[2].startswith("he_create: null argument"), texts
    # and again in the other order, from the engine's second translation unit too (he_fail_text)
    assert he.he_gae(None, None, None, -1, 0.9, 0.9, None, None) != 0
    assert hd.hd_validate_model(None) != 0
    assert "he_gae" in he.he_last_error().decode() and hr.hr_last_error().decode() == texts[1]
    assert hd.hd_last_error().decode() == "model: null model"
    m = C.c_void_p()
    assert hr.hr_create(0, None, 4, C.byref(m)) != 0 and hr.hr_last_error().decode() == "hr_create: null model"
    assert "he_gae" in he.he_last_error().decode()
    # the fourth library: its refusal leaves the other three texts as they are
    before = [f().decode() for f in (hd.hd_last_error, hr.hr_last_error, he.he_last_error)]
    assert hs.hs_solve(None, None, None, None, None, 1, 1, None) != 0
    assert hs.hs_last_error().decode() == "hs_solve: null handle"
    assert [f().decode() for f in (hd.hd_last_error, hr.hr_last_error, he.he_last_error)] == before
