"""Build ``humanoid_amd/libhumanoid_engine.so`` (with its diagnostic twin), the camera-sensor
library ``humanoid_amd/libhumanoid_render.so``, the dynamics-query library
``humanoid_amd/libhumanoid_dynamics.so``, the joint-space solve library
``humanoid_amd/libhumanoid_solve.so`` and the task-space control library
``humanoid_amd/libhumanoid_task.so`` for gfx950 with hipcc (in-tree, they travel with the
repo to the GPU box). Usage: ``python -m humanoid_amd.build [--force]``."""
import glob
import hashlib
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libhumanoid_engine.so")
# diagnostic twin with the physics kernel's per-phase cycle stamps compiled in (tools/phase_profile.py);
# the product library leaves them out (their per-phase branches cost ~1% of the step)
PHASES_LIB = os.path.join(HERE, "libhumanoid_engine_phases.so")
PHASES_DEFS = {"he_physics.hip": ["-DHE_PHASE_STAMPS=1"]}
# the camera-sensor ray caster (include/humanoid_render.h): a library of its own that only reads the
# engine's buffers, so the engine's device code (device_code_id) does not move with it
RENDER_LIB = os.path.join(HERE, "libhumanoid_render.so")
RENDER_SOURCES = [("hr_render.hip", [])]
# the dynamics-query tensors (include/humanoid_dynamics.h: Jacobians, mass matrix, bias force): likewise
# a library of its own that only reads the engine's state buffers
DYNAMICS_LIB = os.path.join(HERE, "libhumanoid_dynamics.so")
DYNAMICS_SOURCES = [("hd_dynamics.hip", [])]
# the joint-space solves (include/humanoid_solve.h: forward dynamics, computed torque, M^-1 on a block of
# vectors): a fourth library, which reads the engine's state buffers and includes the engine's
# register algebra (he_regla.h) without being linked into it
SOLVE_LIB = os.path.join(HERE, "libhumanoid_solve.so")
# no SLP vectorisation, as for the physics kernel: the elimination issues its packed FMAs itself
SOLVE_SOURCES = [("hs_solve.hip", ["-fno-slp-vectorize"])]
# task-space control (include/humanoid_task.h: the task Jacobian rows, J M^-1, the operational-space
# inertia and the task solve in one launch): a fifth product library, which shares the solve kernels'
# path from the state to the factor of M (he_joint_space.h) without being linked to their library
TASK_LIB = os.path.join(HERE, "libhumanoid_task.so")
TASK_SOURCES = [("ht_task.hip", ["-fno-slp-vectorize"])]
BUILD = os.path.join(HERE, "_build")
ARCH = os.environ.get("HE_OFFLOAD_ARCH", "gfx950")

# (source, extra flags): the imitation kernel must evaluate float32 expressions exactly as the
# reference's torch ops do (no FMA contraction); the physics kernel may contract.
SOURCES = [
    ("he_imitation.hip", ["-ffp-contract=off"]),
    # no SLP vectorisation: the compiler's own packed-FP32 pairing costs more moves than it saves;
    # the elimination issues its v_pk_fma_f32 explicitly (he_regla.h)
    # max-ilp scheduling: +1.0% against iterative-ilp (r02 A/B, 3 of 3 passes, bit-identical results),
    # which was +1% against the default (r01); iterative-minreg -4%
    ("he_physics.hip", ["-mllvm", "-amdgpu-mfma-vgpr-form=1", "-fno-slp-vectorize",
                        "-mllvm", "-amdgpu-sched-strategy=max-ilp"]),
    ("he_ingest.hip", []),
    ("he_forces.hip", []),
    ("he_probe.hip", []),  # tests' probe of the vector solves (he_regla.h) in both forms
    ("he_rollout.hip", ["-ffp-contract=off"]),  # GAE: the Cython module's float32 rounding
    ("he_engine.cpp", ["-x", "hip"]),
]
# every header under csrc/ and include/, relative to csrc/: a change to any of them rebuilds every object
HEADERS = sorted(os.path.relpath(h, CSRC) for d in (CSRC, os.path.join(HERE, "..", "include"))
                 for h in glob.glob(os.path.join(d, "*.h")))
# (library, its sources, extra flags by source): a source with extra flags gets an object of its own
# (<source>.phases.o), every other object is shared with the library that built it first
LIBRARIES = [(LIB, SOURCES, {}), (PHASES_LIB, SOURCES, PHASES_DEFS), (RENDER_LIB, RENDER_SOURCES, {}),
             (DYNAMICS_LIB, DYNAMICS_SOURCES, {}), (SOLVE_LIB, SOLVE_SOURCES, {}), (TASK_LIB, TASK_SOURCES, {})]
COMMON = ["--offload-arch=" + ARCH, "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.sep not in c or os.path.exists(c)):
            return c
    raise RuntimeError("hipcc not found")


def compile_command(src, extra=(), device_only=False, out=None):
    """The full hipcc argument list for one source, the one statement of how a kernel source is compiled
    (build() and the tools under tools/ all take it from here): the common flags, the compilation-unit
    id, the source's own flags (SOURCES and its like), then `extra`. src: a file name under csrc/, or a
    path to a copy elsewhere (flags and id follow the file name). device_only: the gfx950 code object
    alone, for the tools that hash or disassemble it. out: the object, by default _build/<name>.o."""
    name = os.path.basename(src)
    flags = {s: f for _, sources, _ in LIBRARIES for s, f in sources}[name]
    # hipcc's default compilation-unit id hashes the source's absolute path into the device
    # symbols of every anonymous-namespace kernel, so device_code_id() would follow the
    # checkout directory; an id from the file name keeps it equal in every checkout
    cuid = "-cuid=" + hashlib.md5(name.encode()).hexdigest()[:16]
    device = ["--cuda-device-only", "--no-gpu-bundle-output"] if device_only else []
    return [_hipcc()] + COMMON + [cuid] + flags + list(extra) + device + \
        ["-c", src if os.path.dirname(src) else os.path.join(CSRC, src), "-o", out or os.path.join(BUILD, name + ".o")]


def _mtime(p):
    return os.path.getmtime(p) if os.path.exists(p) else 0.0


# kernels whose occupancy (waves per SIMD, the compiler's resource report) the build enforces: the
# physics kernel is one wave per env and latency-bound, and at one wave per SIMD it runs ~40 % slower;
# the task kernel is solve_kernel's shape and declares the same two waves
MIN_OCCUPANCY = {"he_physics.hip": ("physics_kernel", 2), "ht_task.hip": ("task_kernel", 2)}
# how many kernels of the TU match the watched name (physics_kernel and physics_kernel_tgs): a report
# that lists fewer fails the build, so neither can drop out of the check unnoticed
MIN_KERNELS = {"he_physics.hip": 2}
# kernels that must not touch scratch memory (no spilled registers, no stack): the render kernels keep
# their primitives in LDS and everything else in registers; the dynamics kernel keeps its matrices in
# named registers and indexes only LDS; the solve kernels (a source names one kernel or a tuple of
# them; a template's instantiations by the name with its mangled argument, render_kernel<false> and
# <true>) hold the mass matrix and its factorisation in registers, within the 256 of two waves per SIMD
NO_SCRATCH = {"hr_render.hip": ("render_kernelILb0", "render_kernelILb1", "rays_kernel"),
              "hd_dynamics.hip": "dynamics_kernel", "hs_solve.hip": ("solve_kernel", "torque_kernel"),
              "ht_task.hip": "task_kernel"}
# further kernels of a source under the same rule, checked after NO_SCRATCH's: a second query family
# compiled in a library's translation unit (hd_centroidal.h in hd_dynamics.hip: the lanes' columns in
# registers, everything indexed in LDS)
NO_SCRATCH_ALSO = {"hd_dynamics.hip": ("centroidal_kernel",)}
# ceilings on the physics kernels' register spills, by exact kernel name: (scratch bytes per lane,
# spilled VGPRs) of the compiler's resource report, no slack (as the occupancy). The TGS kernel's
# spills are a plan, not a by-product: what is parked is the <= 32-row class's columns
# around the rows' register peak and the wide class's columns, fetched back in batches or far ahead
# of their use; an address or a wave-uniform value parked across the position iterations comes back
# in front of the read that needs it, a memory round trip on the step's dependent path, and shows
# here as growth. Round 11 reached 148 B / 36 (its parent: 324 B / 80). The PGS kernel stays at 0.
# The product build only: the stamp twin's per-phase branches move the allocation (148 B / 44).
MAX_SPILLS = {"he_physics.hip": {"physics_kernel_tgs": (148, 36), "physics_kernel": (0, 0)}}


_REPORT_FIELDS = {"Occupancy [waves/SIMD]": "occupancy", "ScratchSize [bytes/lane]": "scratch",
                  "VGPRs Spill": "spilled_vgprs"}


def resource_report(stderr):
    """The compiler's kernel-resource-usage remarks as {function name: block}. A block has "fields", every
    line of the function's report as printed ({"VGPRs": "256", ...}), and as ints "occupancy" (waves per
    SIMD), "scratch" (bytes per lane) and "spilled_vgprs", each None when the report lacks its line."""
    report, block = {}, None
    for ln in stderr.splitlines():
        if "Function Name:" in ln:
            block = report.setdefault(ln.split("Function Name:")[1].split()[0],
                                      dict.fromkeys(_REPORT_FIELDS.values(), None) | {"fields": {}})
            continue
        m = re.search(r"remark:\s+([^:]+):\s+(\S+)", ln)
        if m and block is not None:
            key = m.group(1).strip()
            block["fields"][key] = m.group(2)
            if key in _REPORT_FIELDS and m.group(2).isdigit():
                block[_REPORT_FIELDS[key]] = int(m.group(2))
    return report


def _check_scratch(src, stderr):
    names = NO_SCRATCH.get(os.path.basename(src))
    if not names:
        return
    report = resource_report(stderr)
    names = ((names,) if isinstance(names, str) else tuple(names)) + NO_SCRATCH_ALSO.get(os.path.basename(src), ())
    for name in names:
        scratch = [b["scratch"] for fn, b in report.items() if name in fn and b["scratch"] is not None]
        if not scratch:
            raise RuntimeError(f"{name}: no scratch size in the compiler's resource report")
        if scratch[0] != 0:
            raise RuntimeError(f"{name}: {scratch[0]} bytes/lane of scratch (spills or a stack)")


def _check_spills(src, stderr):
    """Every kernel named in MAX_SPILLS must appear in the resource report, within its ceilings."""
    report = resource_report(stderr)
    for name, (max_bytes, max_vgprs) in MAX_SPILLS.get(os.path.basename(src), {}).items():
        # the mangled name: <length><name>E<argument types>
        got = [(b["scratch"], b["spilled_vgprs"]) for fn, b in report.items() if re.search(r"\d" + name + r"E", fn)]
        if not got or None in got[-1]:
            raise RuntimeError(f"{name}: no scratch size / spill count in the compiler's resource report")
        got = got[-1]
        if got[0] > max_bytes or got[1] > max_vgprs:
            raise RuntimeError(f"{name}: {got[0]} bytes/lane of scratch, {got[1]} spilled VGPRs; the ceiling is "
                               f"{max_bytes} / {max_vgprs} (list the kernel's scratch reloads: DESIGN §4.1)")


def _check_occupancy(src, stderr):
    """Every kernel of the TU whose name contains the watched name (the physics TU: physics_kernel and
    physics_kernel_tgs) must reach the occupancy."""
    want = MIN_OCCUPANCY.get(os.path.basename(src))
    if not want:
        return
    name, waves = want
    watched = {fn: b["occupancy"] for fn, b in resource_report(stderr).items() if name in fn}
    for fn, occ in watched.items():
        if occ is None:
            raise RuntimeError(f"{fn}: no occupancy line in the compiler's resource report")
        if occ < waves:
            raise RuntimeError(f"{fn}: occupancy {occ} waves/SIMD < {waves} "
                               "(register pressure; see the resource report)")
    expected = MIN_KERNELS.get(os.path.basename(src), 1)
    if len(watched) < expected:
        raise RuntimeError(f"{name}: {len(watched)} kernel(s) in the compiler's resource report, {expected} expected")


def _compile(hipcc, cmd, src, o, force, hdr_time, verbose, product=False):
    stamp = o + ".cmd"  # a flag change rebuilds too
    same_cmd = os.path.exists(stamp) and open(stamp).read() == " ".join(cmd)
    if force or not same_cmd or _mtime(o) < max(_mtime(src), hdr_time):
        if verbose:
            print(" ".join(cmd))
        if os.path.basename(src) in MIN_OCCUPANCY or os.path.basename(src) in NO_SCRATCH:
            cmd = cmd + ["-Rpass-analysis=kernel-resource-usage"]
        # a failed compile or occupancy check leaves neither the object nor the stamp behind, so the
        # next build cannot mistake a rejected object for an up-to-date one
        _discard(o, stamp)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            _discard(o, stamp)
            raise RuntimeError(f"hipcc failed for {os.path.basename(src)}:\n{r.stderr}")
        try:
            _check_occupancy(src, r.stderr)
            _check_scratch(src, r.stderr)
            if product:
                _check_spills(src, r.stderr)
        except RuntimeError:
            _discard(o, stamp)
            raise
        cmd = cmd[:-1] if cmd[-1] == "-Rpass-analysis=kernel-resource-usage" else cmd
        with open(stamp, "w") as f:
            f.write(" ".join(cmd))
        return True
    return False


def _discard(*paths):
    for p in paths:
        if os.path.exists(p):
            os.remove(p)


def _link(hipcc, lib, objs, force):
    if force or _mtime(lib) < max(_mtime(o) for o in objs):
        cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", lib] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stderr}")


def build(force=False, verbose=False):
    os.makedirs(BUILD, exist_ok=True)
    hipcc = _hipcc()
    hdr_time = max(_mtime(os.path.join(CSRC, h)) for h in HEADERS)
    for lib, sources, defs in LIBRARIES:
        objs = []
        for src, _ in sources:
            o = os.path.join(BUILD, src + (".phases.o" if src in defs else ".o"))
            objs.append(o)
            # an object shared with an earlier library was forced there; the ceilings on the register
            # spills hold for the product objects only
            _compile(hipcc, compile_command(src, defs.get(src, ()), out=o), os.path.join(CSRC, src), o,
                     force and (not defs or src in defs), hdr_time, verbose, product=src not in defs)
        _link(hipcc, lib, objs, force)
    return LIB


def device_code_id(lib=LIB):
    """sha256[:16] of the library's embedded device code (the ELF `.hip_fatbin` section: every gfx950
    code object linked in). Host-only changes leave it equal; any kernel change moves it. Measurement
    records (tests/test_full_size.py) store it, and bench.py reports a record as stale when it does not
    match the library it loaded."""
    import hashlib
    import struct
    with open(lib, "rb") as f:
        data = f.read()
    if data[:4] != b"\x7fELF" or data[4] != 2:
        raise RuntimeError(f"{lib}: not an ELF64 file")
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)

    def sec(i):
        name, _, _, _, off, size = struct.unpack_from("<IIQQQQ", data, shoff + i * shentsize)
        return name, off, size
    _, stroff, _ = sec(shstrndx)
    for i in range(shnum):
        name, off, size = sec(i)
        end = data.index(b"\0", stroff + name)
        if data[stroff + name:end] == b".hip_fatbin":
            return hashlib.sha256(data[off:off + size]).hexdigest()[:16]
    raise RuntimeError(f"{lib}: no .hip_fatbin section")


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
