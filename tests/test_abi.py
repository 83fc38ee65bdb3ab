"""CPU checks of the drop-in boundary: the C-ABI library loads and exports every symbol the
header declares; ctypes struct layouts match the header's sizes; host-side model/topology logic."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "humanoid_engine.h")


def declared_symbols():
    import glob
    text = "".join(open(h).read() for h in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))))
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(he_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from humanoid_amd import engine
    lib_path = engine.LIB_PATH
    if not os.path.exists(lib_path):
        from humanoid_amd import build
        build.build()
    lib = C.CDLL(lib_path)  # loads without a GPU
    syms = declared_symbols()
    assert len(syms) >= 20
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    assert set(syms) == set(engine.HE_SYMBOLS)
    lib.he_version.restype = C.c_int
    assert lib.he_version() == 1
    lib.he_hash_uniform.restype = C.c_float
    lib.he_hash_uniform.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    from oracle import oracle as O
    for s, st, e in [(0, 0, 0), (1, 7, 4095), (123456789, 1 << 40, 17)]:
        assert lib.he_hash_uniform(s, st, e) == O.hash_uniform(s, st, e)


def test_build_tracks_every_kernel_header():
    """build.build() rebuilds when a header changes only if the header is in build.HEADERS: every
    header a kernel source includes must be listed (an unlisted one once left a stale library)."""
    import glob
    from humanoid_amd import build
    csrc = os.path.join(ROOT, "humanoid_amd", "csrc")
    tracked = {os.path.normpath(os.path.join(csrc, h)) for h in build.HEADERS}
    for src in glob.glob(os.path.join(csrc, "*")):
        for inc in re.findall(r'#include\s+"([^"]+)"', open(src).read()):
            path = os.path.normpath(os.path.join(csrc, inc))
            assert path in tracked, f"{os.path.basename(src)} includes {inc}, not in build.HEADERS"


def test_errors_are_reported_without_gpu():
    from humanoid_amd import _abi, engine
    lib = engine.load_library()
    h = C.c_void_p()
    p = _abi.default_sim_params()
    rc = lib.he_create(C.byref(p), 0, C.byref(h))
    assert rc != 0
    assert lib.he_last_error().decode()


def test_struct_sizes_match_header(tmp_path):
    from humanoid_amd import _abi
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "humanoid_engine.h"\n#include "humanoid_rollout.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu\\n",'
                   "sizeof(he_model),sizeof(he_sim_params),sizeof(he_imitation_params),sizeof(he_env_motion),"
                   "sizeof(he_rollout_field),sizeof(he_rollout_index));}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [C.sizeof(_abi.HeModel), C.sizeof(_abi.HeSimParams),
                                     C.sizeof(_abi.HeImitationParams), C.sizeof(_abi.HeEnvMotion),
                                     C.sizeof(_abi.HeRolloutField), C.sizeof(_abi.HeRolloutIndex)]


def test_model_blob(model):
    from humanoid_amd import _abi
    hm = _abi.make_model(model)
    assert hm.num_pairs == 245
    assert abs(sum(hm.mass) - 73.995) < 1e-2
    assert list(hm.parents)[:5] == [-1, 0, 1, 2, 3]


def test_mjcf_roundtrip_matches_baked_json(model):
    xml = "/root/reference/packages/puffer-phc/puffer_phc/assets/smpl_humanoid.xml"
    if not os.path.exists(xml):
        pytest.skip("reference asset not present (GPU box)")
    from humanoid_amd.model import parse_mjcf
    m = parse_mjcf(xml)
    np.testing.assert_allclose(m.local_pos, model.local_pos)
    np.testing.assert_allclose(m.mass, model.mass)
    np.testing.assert_allclose(m.inertia, model.inertia)


def test_occupancy_guard_removes_the_rejected_object(tmp_path, monkeypatch):
    """build._compile must not leave an object (or its command stamp) behind when the occupancy check
    rejects it: the next build would otherwise see an up-to-date object and skip the check."""
    import subprocess
    import types
    from humanoid_amd import build
    from resource_reports import at_budget
    src = tmp_path / "he_physics.hip"
    src.write_text("// fake")
    o = str(tmp_path / "he_physics.hip.o")
    stamp = o + ".cmd"
    remark = at_budget("he_physics.hip", {"physics_kernel_tgs": {"occupancy": 1}})
    ran = []

    def fake_run(cmd, capture_output=True, text=True):
        ran.append(cmd)
        out = cmd[cmd.index("-o") + 1]
        with open(out, "w") as f:
            f.write("object")
        return types.SimpleNamespace(returncode=0, stderr=remark, stdout="")

    monkeypatch.setattr(subprocess, "run", fake_run)
    cmd = ["hipcc", "-c", str(src), "-o", o]
    with open(stamp, "w") as f:  # a stamp from an earlier build with the same command
        f.write(" ".join(cmd))
    with pytest.raises(RuntimeError, match="physics_kernel_tgs: occupancy 1 waves/SIMD < 2"):
        build._compile(cmd, str(src), o, True, 0.0, False)
    assert not os.path.exists(o) and not os.path.exists(stamp)
    # the twin is held to the occupancy too
    with pytest.raises(RuntimeError, match="physics_kernel_tgs: occupancy 1 waves/SIMD < 2"):
        build._compile(cmd, str(src), o, True, 0.0, False, product=False)
    assert not os.path.exists(o) and not os.path.exists(stamp)
    # a passing report keeps the object and writes the stamp: the command as given, run with the report's flag
    full = remark = at_budget("he_physics.hip")
    assert build._compile(cmd, str(src), o, True, 0.0, False)
    assert os.path.exists(o) and open(stamp).read() == " ".join(cmd)
    assert ran[-1] == cmd + ["-Rpass-analysis=kernel-resource-usage"]
    assert not build._compile(cmd, str(src), o, False, 0.0, False)  # up to date
    # a kernel whose report has no occupancy line, or a missing kernel, fails too
    remark = at_budget("he_physics.hip", {"physics_kernel": {"occupancy": None}})
    with pytest.raises(RuntimeError, match="physics_kernel: no occupancy line"):
        build._compile(cmd, str(src), o, True, 0.0, False)
    assert not os.path.exists(o) and not os.path.exists(stamp)
    remark = at_budget("he_physics.hip", without=["physics_kernel_tgs"])
    with pytest.raises(RuntimeError, match="physics_kernel_tgs: not in the compiler's resource report"):
        build._compile(cmd, str(src), o, True, 0.0, False)
    # a failed compile leaves nothing behind either, and a source without entries is compiled without the report
    remark = full
    assert build._compile(cmd, str(src), o, True, 0.0, False)
    monkeypatch.setattr(subprocess, "run", lambda cmd, **kw: types.SimpleNamespace(returncode=1, stderr="boom", stdout=""))
    with pytest.raises(RuntimeError, match="hipcc failed for he_physics.hip"):
        build._compile(cmd, str(src), o, True, 0.0, False)
    assert not os.path.exists(o) and not os.path.exists(stamp)
    monkeypatch.setattr(subprocess, "run", fake_run)
    remark = ""
    other = str(tmp_path / "he_ingest.hip")
    assert build._compile(["hipcc", "-c", other, "-o", o], other, o, True, 0.0, False)
    assert ran[-1] == ["hipcc", "-c", other, "-o", o]


def test_spill_ceilings_read_the_named_kernel():
    """build.check_resources holds each physics kernel to its own ceilings, by exact name: physics_kernel
    never reads physics_kernel_tgs's block, and a kernel missing from the report fails."""
    from humanoid_amd import build
    from resource_reports import at_budget
    table = build.BUDGETS["he_physics.hip"]
    _, ceil_b, ceil_v = table["physics_kernel_tgs"]
    assert (ceil_b, ceil_v) == (148, 36) and table["physics_kernel"] == (2, 0, 0)
    assert table["physics_kernel_ext"] == (2, 0, 0) and table["physics_kernel_tgs_ext"] == (2, 156, 38)
    assert table["physics_order_kernel"] == table["warm_tu_kernel"] == (None, 0, None) and len(table) == 6

    def check(changes=None, **kw):
        build.check_resources("he_physics.hip", at_budget("he_physics.hip", changes, **kw))

    # both orders of the two blocks: the PGS kernel at 0 / 0, the TGS kernel at its ceiling
    check()
    check(order=["physics_kernel_tgs", "physics_kernel"] + [k for k in table if k not in ("physics_kernel_tgs", "physics_kernel")])
    with pytest.raises(RuntimeError, match=rf"physics_kernel_tgs: {ceil_b + 1} bytes/lane of scratch, {ceil_v} spilled"):
        check({"physics_kernel_tgs": {"scratch": ceil_b + 1}})
    with pytest.raises(RuntimeError, match=rf"physics_kernel_tgs: {ceil_b} bytes/lane of scratch, {ceil_v + 1} spilled"):
        check({"physics_kernel_tgs": {"spilled_vgprs": ceil_v + 1}})
    with pytest.raises(RuntimeError, match="physics_kernel_tgs: not in the compiler's resource report"):
        check(without=["physics_kernel_tgs"])
    with pytest.raises(RuntimeError, match="physics_kernel: not in the compiler's resource report"):
        check(without=["physics_kernel"])
    # a block without its spill line, or its scratch line, is a missing line, not a pass
    for line in ("spilled_vgprs", "scratch"):
        with pytest.raises(RuntimeError, match="physics_kernel_tgs: no scratch size / spill count"):
            check({"physics_kernel_tgs": {line: None}})
    # each figure of each kernel, over its ceiling by one, fails and names its kernel alone
    for kernel, (_, b, v) in table.items():
        for over in ({"scratch": b + 1}, {"spilled_vgprs": v + 1} if v is not None else {"scratch": b + 2}):
            with pytest.raises(RuntimeError) as e:
                check({kernel: over})
            assert str(e.value).startswith(f"{kernel}: {over.get('scratch', b)} bytes/lane of scratch")
    # only the TGS kernel exceeds: the error names it, in either order of the blocks, and never the PGS kernel
    for order in (list(table), list(table)[::-1]):
        with pytest.raises(RuntimeError) as e:
            check({"physics_kernel_tgs": {"scratch": ceil_b + 8, "spilled_vgprs": ceil_v + 2}}, order=order)
        assert str(e.value).startswith(f"physics_kernel_tgs: {ceil_b + 8} bytes/lane of scratch, {ceil_v + 2} spilled VGPRs")
        assert f"{ceil_b} / {ceil_v}" in str(e.value) and "DESIGN §4.1" in str(e.value)
    # sources without entries are not checked
    build.check_resources("he_ingest.hip", "")


def test_compile_command_is_the_builds():
    """build.compile_command gives, for every object of the six libraries, the line build() has always
    written into the object's .cmd stamp (so a tree built before recompiles nothing for the flags' sake),
    and tools/build_variant.py's line for the physics TU is the product's but for the object."""
    import hashlib
    import sys
    from humanoid_amd import build
    common = ["--offload-arch=" + build.ARCH, "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function"]
    # every source's flags spelled out here, not read from the table the build reads
    engine = [("he_imitation.hip", ["-ffp-contract=off"]),
              ("he_physics.hip", ["-mllvm", "-amdgpu-mfma-vgpr-form=1", "-fno-slp-vectorize",
                                  "-mllvm", "-amdgpu-sched-strategy=max-ilp"]),
              ("he_ingest.hip", []), ("he_forces.hip", []), ("he_probe.hip", []),
              ("he_rollout.hip", ["-ffp-contract=off"]), ("he_engine.cpp", ["-x", "hip"])]
    libraries = [("libhumanoid_engine.so", engine, {}),
                 ("libhumanoid_engine_phases.so", engine, {"he_physics.hip": ["-DHE_PHASE_STAMPS=1"]}),
                 ("libhumanoid_render.so", [("hr_render.hip", [])], {}),
                 ("libhumanoid_dynamics.so", [("hd_dynamics.hip", [])], {}),
                 ("libhumanoid_solve.so", [("hs_solve.hip", ["-fno-slp-vectorize"])], {}),
                 ("libhumanoid_task.so", [("ht_task.hip", ["-fno-slp-vectorize"])], {})]
    assert [(lib.path, lib.sources, lib.defs) for lib in build.LIBRARIES.values()] == \
        [(os.path.join(build.HERE, name), sources, defs) for name, sources, defs in libraries]
    n = 0
    for lib, (_, sources, defs) in zip(build.LIBRARIES.values(), libraries):
        assert len(lib.objects()) == len(sources)
        for (src, flags), (obj_src, obj) in zip(sources, lib.objects()):
            o = os.path.join(build.BUILD, src + (".phases.o" if src in defs else ".o"))
            assert (obj_src, obj) == (src, o)
            want = [build._hipcc()] + common + ["-cuid=" + hashlib.md5(src.encode()).hexdigest()[:16]] + flags + \
                defs.get(src, []) + ["-c", os.path.join(build.CSRC, src), "-o", o]
            assert " ".join(build.compile_command(src, defs.get(src, ()), out=o)) == " ".join(want)
            n += 1
    assert n == 18
    # the physics TU's line spelled out, and the default object
    phys = os.path.join(build.CSRC, "he_physics.hip")
    assert " ".join(build.compile_command("he_physics.hip")) == (
        f"{build._hipcc()} --offload-arch={build.ARCH} -O3 -fPIC -std=c++17 -Wall -Wno-unused-function "
        "-cuid=a5c8526841ebfadf -mllvm -amdgpu-mfma-vgpr-form=1 -fno-slp-vectorize -mllvm "
        f"-amdgpu-sched-strategy=max-ilp -c {phys} -o {os.path.join(build.BUILD, 'he_physics.hip.o')}")
    # the tools' code object: the same line with the device-only pair in front of -c; a copy of the source
    # elsewhere keeps the flags and the id of its file name
    dev = build.compile_command("/elsewhere/he_physics.hip", ["-DX=1"], device_only=True, out="k.co")
    assert dev[-7:] == ["-DX=1", "--cuda-device-only", "--no-gpu-bundle-output", "-c", "/elsewhere/he_physics.hip", "-o", "k.co"]
    assert dev[:-7] == build.compile_command("he_physics.hip")[:-4]
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import build_variant
    finally:
        sys.path.pop(0)
    cmd, obj = build_variant.variant_command("same", "he_physics.hip", [])
    product = build.compile_command("he_physics.hip")
    assert cmd[:-1] == product[:-1] and cmd[-1] == obj != product[-1]
    # a variant's sched-strategy replaces the product's
    cmd, _ = build_variant.variant_command("s", "he_physics.hip", ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"])
    assert [c for c in cmd if c.startswith("-amdgpu-sched-strategy=")] == ["-amdgpu-sched-strategy=iterative-ilp"]
    assert cmd.count("-mllvm") == product.count("-mllvm")


def test_physics_headers_stand_alone(tmp_path):
    """Each he_phys_*.h includes what it uses: a source that includes that header alone passes the
    compiler's front end with the physics TU's own compile line."""
    import glob
    import shutil
    from humanoid_amd import build
    if shutil.which(build._hipcc()) is None:
        pytest.skip("hipcc not present")
    headers = sorted(glob.glob(os.path.join(build.CSRC, "he_phys_*.h")))
    assert len(headers) >= 8
    runs = []
    for h in headers:  # the front ends side by side
        d = tmp_path / os.path.basename(h)
        d.mkdir()
        src = d / "he_physics.hip"  # the flags follow the file name
        src.write_text(f'#include "{h}"\n')
        cmd = build.compile_command(str(src), ["-fsyntax-only"], device_only=True, out=str(d / "none.o"))
        runs.append((h, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    for h, p in runs:
        _, err = p.communicate()
        assert p.returncode == 0, f"{os.path.basename(h)} does not compile on its own:\n{err}"
