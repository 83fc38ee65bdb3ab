"""Per-phase register spills of the physics kernel under a waves-per-SIMD bound (diagnostic for the
occupancy plan): the stamp build of he_physics.hip compiled with -DHE_MIN_WAVES=W (the
launch bound: 256 / W VGPRs), disassembled and split at its s_memtime stamps as in
tools/isa_phase_counts.py; per phase the scratch stores and loads the allocator inserted, and the
kernel's resource report.

  python tools/spill_map.py [W] [KERNEL]      (default 4, physics_kernel; physics_kernel_tgs: the TGS one)
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from humanoid_amd import build as B  # noqa: E402
from phase_profile import PHASES  # noqa: E402

LLVM = "/opt/rocm/lib/llvm/bin"


def main():
    w = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    kname = sys.argv[2] if len(sys.argv) > 2 else "physics_kernel"
    with tempfile.TemporaryDirectory() as td:
        co = os.path.join(td, "k.co")
        extra = B.LIBRARIES["engine_phases"].defs["he_physics.hip"] + [f"-DHE_MIN_WAVES={w}", B.REPORT_FLAG]
        r = subprocess.run(B.compile_command("he_physics.hip", extra, device_only=True, out=co),
                           check=True, capture_output=True, text=True)
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True,
                             capture_output=True, text=True).stdout
    # the kernel's block of the resource report, by its exact name
    report = B.kernel_reports(r.stderr).get(kname, {}).get("fields", {})
    L = dis.split("\n")
    # the kernel's own disassembly: from its label to the next function label
    start = next(i for i, ln in enumerate(L) if re.search(r"\d" + kname + r"E\w*>:", ln))
    end = next((i for i in range(start + 1, len(L)) if re.match(r"^[0-9a-f]+ <", L[i])), len(L))
    L = L[start:end]
    cuts = [i for i, ln in enumerate(L) if "s_memtime" in ln]
    phases = {}
    for a, b in zip(cuts, cuts[1:]):
        slot = None
        for ln in L[b:b + 80]:
            if "global_atomic_add" in ln:
                m = re.search(r"offset:(\d+)", ln)
                slot = int(m.group(1)) // 8 if m else 0
                break
        name = PHASES[slot] if slot is not None and slot < len(PHASES) else f"slot {slot}"
        seg = L[a:b]
        c = phases.setdefault(name, {"scratch_stores": 0, "scratch_loads": 0, "instructions": 0})
        c["scratch_stores"] += sum("scratch_store" in ln for ln in seg)
        c["scratch_loads"] += sum("scratch_load" in ln for ln in seg)
        c["instructions"] += sum(1 for ln in seg if re.match(r"\s+[a-z_0-9]+\s", ln))
    print(json.dumps({"waves_per_simd_bound": w, "resources": report, "phases": phases}, indent=1))


if __name__ == "__main__":
    main()
