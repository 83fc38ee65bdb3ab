"""Build the project's shared libraries (LIBRARIES: the engine with its diagnostic twin, and the render,
dynamics, solve and task libraries) for gfx950 with hipcc, in-tree (they travel with the repo to the GPU
box), and hold every kernel of the checked sources to its resource budget (BUDGETS, check_resources).
Usage: ``python -m humanoid_amd.build [--force]``."""
import glob
import hashlib
import os
import re
import subprocess
import sys
from typing import NamedTuple, Optional

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
BUILD = os.path.join(HERE, "_build")
ARCH = os.environ.get("HE_OFFLOAD_ARCH", "gfx950")


class Library(NamedTuple):
    name: str        # the file is libhumanoid_<name>.so, beside this module
    sources: list    # (source under csrc/, its extra flags)
    defs: dict = {}  # further definitions by source: such a source gets an object of its own (<source>.phases.o)

    @property
    def path(self):
        return os.path.join(HERE, f"libhumanoid_{self.name}.so")

    def objects(self):
        """(source, its object): an object without further definitions is shared with every library that lists the source."""
        return [(s, os.path.join(BUILD, s + (".phases.o" if s in self.defs else ".o"))) for s, _ in self.sources]


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
# the one statement of the libraries, by name; the bindings take their LIB_PATH from here
LIBRARIES = {lib.name: lib for lib in (
    Library("engine", SOURCES),
    # diagnostic twin with the physics kernel's per-phase cycle stamps compiled in (tools/phase_profile.py);
    # the product library leaves them out (their per-phase branches cost ~1% of the step)
    Library("engine_phases", SOURCES, {"he_physics.hip": ["-DHE_PHASE_STAMPS=1"]}),
    # the camera-sensor ray caster (include/humanoid_render.h): a library of its own that only reads the
    # engine's buffers, so the engine's device code (device_code_id) does not move with it
    Library("render", [("hr_render.hip", [])]),
    # the dynamics-query tensors (include/humanoid_dynamics.h: Jacobians, mass matrix, bias force): likewise
    # a library of its own that only reads the engine's state buffers
    Library("dynamics", [("hd_dynamics.hip", [])]),
    # the joint-space solves (include/humanoid_solve.h: forward dynamics, computed torque, M^-1 on a block of
    # vectors): a fourth library, which reads the engine's state buffers and includes the engine's
    # register algebra (he_regla.h) without being linked into it
    # no SLP vectorisation, as for the physics kernel: the elimination issues its packed FMAs itself.
    # The joint-reaction queries (include/humanoid_wrench.h, the hw_ entry points) are a second family of
    # this library: device code in csrc/hs_wrench.h, run by torque_kernel itself; the dynamics derivatives
    # (include/humanoid_derivatives.h, the hg_ entry points) a third, in csrc/hs_derivs.h
    Library("solve", [("hs_solve.hip", ["-fno-slp-vectorize"])]),
    # task-space control (include/humanoid_task.h: the task Jacobian rows, J M^-1, the operational-space
    # inertia and the task solve in one launch): a fifth product library, which shares the solve kernels'
    # path from the state to the factor of M (he_joint_space.h) without being linked to their library
    Library("task", [("ht_task.hip", ["-fno-slp-vectorize"])]),
)}
LIB = LIBRARIES["engine"].path  # the product: what build() returns and device_code_id() reads by default
# every header under csrc/ and include/, relative to csrc/: a change to any of them rebuilds every object
HEADERS = sorted(os.path.relpath(h, CSRC) for d in (CSRC, os.path.join(HERE, "..", "include"))
                 for h in glob.glob(os.path.join(d, "*.h")))
COMMON = ["--offload-arch=" + ARCH, "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function"]
REPORT_FLAG = "-Rpass-analysis=kernel-resource-usage"


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.sep not in c or os.path.exists(c)):
            return c
    raise RuntimeError("hipcc not found")


def compile_command(src, extra=(), device_only=False, out=None):
    """The full hipcc argument list for one source, the one statement of how a kernel source is compiled
    (build() and the tools under tools/ all take it from here): the common flags, the compilation-unit
    id, the source's own flags (LIBRARIES), then `extra`. src: a file name under csrc/, or a
    path to a copy elsewhere (flags and id follow the file name). device_only: the gfx950 code object
    alone, for the tools that hash or disassemble it. out: the object, by default _build/<name>.o."""
    name = os.path.basename(src)
    flags = {s: f for lib in LIBRARIES.values() for s, f in lib.sources}[name]
    # hipcc's default compilation-unit id hashes the source's absolute path into the device
    # symbols of every anonymous-namespace kernel, so device_code_id() would follow the
    # checkout directory; an id from the file name keeps it equal in every checkout
    cuid = "-cuid=" + hashlib.md5(name.encode()).hexdigest()[:16]
    device = ["--cuda-device-only", "--no-gpu-bundle-output"] if device_only else []
    return [_hipcc()] + COMMON + [cuid] + flags + list(extra) + device + \
        ["-c", src if os.path.dirname(src) else os.path.join(CSRC, src), "-o", out or os.path.join(BUILD, name + ".o")]


def _mtime(p):
    return os.path.getmtime(p) if os.path.exists(p) else 0.0


class Budget(NamedTuple):
    """What the build holds one kernel to, figures of the compiler's resource report; None: not held."""
    min_waves: Optional[int] = None          # occupancy, waves per SIMD: binds every object
    max_scratch: Optional[int] = None        # scratch bytes per lane: binds the product objects
    max_spilled_vgprs: Optional[int] = None  # likewise


# source -> kernel (its name as the source writes it, a template's with its arguments) -> budget. Every
# kernel of a source listed here has an entry: check_resources fails on a function the table does not name.
BUDGETS = {
    # occupancy: the physics kernel is one wave per env and latency-bound, and at one wave per SIMD it
    # runs ~40 % slower. Ceilings on the register spills, no slack (as the occupancy): the TGS kernel's
    # spills are a plan, not a by-product: what is parked is the <= 32-row class's columns
    # around the rows' register peak and the wide class's columns, fetched back in batches or far ahead
    # of their use; an address or a wave-uniform value parked across the position iterations comes back
    # in front of the read that needs it, a memory round trip on the step's dependent path, and shows
    # here as growth. Round 11 reached 148 B / 36 (its parent: 324 B / 80). The PGS kernel stays at 0.
    # The EXT kernels (a wrench or an actuation force is set) at what the same source compiles to.
    # The product build only: the stamp twin's per-phase branches move the allocation (148 B / 44).
    "he_physics.hip": {"physics_kernel": Budget(2, 0, 0), "physics_kernel_tgs": Budget(2, 148, 36),
                       "physics_kernel_ext": Budget(2, 0, 0), "physics_kernel_tgs_ext": Budget(2, 156, 38),
                       "physics_order_kernel": Budget(max_scratch=0), "warm_tu_kernel": Budget(max_scratch=0)},
    # no scratch memory (no spilled registers, no stack): the render kernels keep their primitives in LDS
    # and everything else in registers
    "hr_render.hip": {"render_kernel<false>": Budget(max_scratch=0), "render_kernel<true>": Budget(max_scratch=0),
                      "rays_kernel": Budget(max_scratch=0)},
    # the dynamics kernel keeps its matrices in named registers and indexes only LDS; the second query
    # family of the translation unit (hd_centroidal.h) the lanes' columns in registers, everything indexed in LDS
    "hd_dynamics.hip": {"dynamics_kernel": Budget(max_scratch=0), "centroidal_kernel": Budget(max_scratch=0)},
    # the solve kernels hold the mass matrix and its factorisation in registers, within the 256 of two
    # waves per SIMD; the second query family of the translation unit (hs_wrench.h) adds no kernel: it is
    # torque_kernel's run-time extension, staged in LDS that is dead by then; the third (hs_derivs.h) likewise,
    # its per-lane tangents in dynamic LDS that only its own launch asks for
    "hs_solve.hip": {"solve_kernel": Budget(max_scratch=0), "torque_kernel": Budget(max_scratch=0)},
    # the task kernel is solve_kernel's shape and declares the same two waves
    "ht_task.hip": {"task_kernel": Budget(min_waves=2, max_scratch=0)},
}


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


def kernel_name(symbol):
    """A kernel's name as its source writes it, out of its symbol: the anonymous-namespace Itanium form
    _ZN12_GLOBAL__N_1<length><name>..., a template's instantiation with its literal arguments
    (...13render_kernelILb0EE... is render_kernel<false>); any other symbol as it is."""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", symbol)
    if not m:
        return symbol
    end = m.end() + int(m.group(1))
    name, args = symbol[m.end():end], re.match(r"I((?:L[a-z]n?\d+E)+)E", symbol[end:])
    if args:  # L<type><value>E each: a bool as the source spells it, an integer by its value
        values = [{"b0": "false", "b1": "true"}.get(a, a[1:].replace("n", "-"))
                  for a in re.findall(r"L([a-z]n?\d+)E", args.group(1))]
        name += "<" + ", ".join(values) + ">"
    elif symbol[end:end + 1] == "I":  # arguments this does not read: the mangling stays, and names no entry
        name += symbol[end:]
    return name


def kernel_reports(stderr):
    """resource_report's blocks by kernel_name."""
    return {kernel_name(fn): block for fn, block in resource_report(stderr).items()}


def check_resources(src, stderr, product=True):
    """Hold the compiler's resource report of one object to BUDGETS[source]: the report's functions are
    exactly the table's kernels, and each kernel keeps within its budget; a held figure whose line the
    report lacks fails. The scratch and spill ceilings bind the product objects only."""
    budgets = BUDGETS.get(os.path.basename(src))
    if not budgets:
        return
    report = kernel_reports(stderr)
    for name in report:
        if name not in budgets:
            raise RuntimeError(f"{name}: a function of {os.path.basename(src)} that build.BUDGETS does not name")
    for name, want in budgets.items():
        if name not in report:
            raise RuntimeError(f"{name}: not in the compiler's resource report")
        occ, scratch, spilled = (report[name][k] for k in ("occupancy", "scratch", "spilled_vgprs"))
        if want.min_waves is not None:
            if occ is None:
                raise RuntimeError(f"{name}: no occupancy line in the compiler's resource report")
            if occ < want.min_waves:
                raise RuntimeError(f"{name}: occupancy {occ} waves/SIMD < {want.min_waves} "
                                   "(register pressure; see the resource report)")
        if not product or want.max_scratch is None:
            continue
        if want.max_spilled_vgprs is None:
            if scratch is None:
                raise RuntimeError(f"{name}: no scratch size in the compiler's resource report")
            if scratch > want.max_scratch:
                raise RuntimeError(f"{name}: {scratch} bytes/lane of scratch (spills or a stack); "
                                   f"the ceiling is {want.max_scratch}")
        else:
            if scratch is None or spilled is None:
                raise RuntimeError(f"{name}: no scratch size / spill count in the compiler's resource report")
            if scratch > want.max_scratch or spilled > want.max_spilled_vgprs:
                raise RuntimeError(f"{name}: {scratch} bytes/lane of scratch, {spilled} spilled VGPRs; the ceiling is "
                                   f"{want.max_scratch} / {want.max_spilled_vgprs} "
                                   "(list the kernel's scratch reloads: DESIGN §4.1)")


def _compile(cmd, src, o, force, hdr_time, verbose, product=True):
    stamp = o + ".cmd"  # a flag change rebuilds too
    same_cmd = os.path.exists(stamp) and open(stamp).read() == " ".join(cmd)
    if same_cmd and not force and _mtime(o) >= max(_mtime(src), hdr_time):
        return False
    if verbose:
        print(" ".join(cmd))
    # a failed compile or resource check leaves neither the object nor the stamp behind, so the
    # next build cannot mistake a rejected object for an up-to-date one
    _discard(o, stamp)
    # the report is asked for exactly where it is checked; the flag is not part of the stamp
    r = subprocess.run(cmd + [REPORT_FLAG] if os.path.basename(src) in BUDGETS else cmd, capture_output=True, text=True)
    try:
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {os.path.basename(src)}:\n{r.stderr}")
        check_resources(src, r.stderr, product)
    except RuntimeError:
        _discard(o, stamp)
        raise
    with open(stamp, "w") as f:
        f.write(" ".join(cmd))
    return True


def _discard(*paths):
    for p in paths:
        if os.path.exists(p):
            os.remove(p)


def _link(lib, objs, force):
    if force or _mtime(lib) < max(_mtime(o) for o in objs):
        cmd = [_hipcc(), "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", lib] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stderr}")


def build(force=False, verbose=False):
    os.makedirs(BUILD, exist_ok=True)
    hdr_time = max(_mtime(os.path.join(CSRC, h)) for h in HEADERS)
    visited = set()  # objects of this call: one shared by two libraries is compiled (or forced) once
    for lib in LIBRARIES.values():
        for src, o in lib.objects():
            if o not in visited:
                visited.add(o)
                _compile(compile_command(src, lib.defs.get(src, ()), out=o), os.path.join(CSRC, src), o,
                         force, hdr_time, verbose, product=src not in lib.defs)
        _link(lib.path, [o for _, o in lib.objects()], force)
    return LIB


def device_code_id(lib=LIB):
    """sha256[:16] of the library's embedded device code (the ELF `.hip_fatbin` section: every gfx950
    code object linked in). Host-only changes leave it equal; any kernel change moves it. Measurement
    records (tests/test_full_size.py) store it, and bench.py reports a record as stale when it does not
    match the library it loaded."""
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
