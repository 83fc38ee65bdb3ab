"""Static control-skeleton counts of the TGS physics kernel (diagnostic, DESIGN §4.1 "Control
skeleton"): a device-only code object of he_physics.hip (the product flags of humanoid_amd/build.py)
is disassembled, which resolves the vector solves' assembler `.if` alternates, and its instructions
are counted for physics_kernel_tgs as a whole and for the <= 32-row position-iteration loop alone:
total, SALU, s_and_saveexec, s_or exec restores, branches by kind, s_waitcnt.

The iteration loops are the innermost natural loops (a backward branch and its target) that run
the serial solves under a raised s_setprio: the <= 32-row class (solve_tgs<32>: 48 sweep rows, one
v_med3_f32 each), the wide class (111 sweep rows) and the iterations without rows (none). A loop's span runs from its head
to its backward branch, so a rare block that the layout moved behind the loop is not counted in it.

  python tools/control_skeleton.py [CODE_OBJECT] [-- extra hipcc flags]
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from humanoid_amd import build as B  # noqa: E402

LLVM = "/opt/rocm/lib/llvm/bin"
NAMES = ["<=32-row loop", "wide loop", "free loop"]
KEYS = ["total", "valu", "salu", "s_and_saveexec", "s_or_exec", "s_andn2_exec", "lds", "vmem", "s_waitcnt", "s_nop",
        "branches", "s_cbranch_execz", "s_cbranch_execnz", "s_cbranch_vccz", "s_cbranch_vccnz", "s_cbranch_scc0",
        "s_cbranch_scc1", "s_branch"]


def disassemble(co):
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True,
                         capture_output=True, text=True).stdout
    kernels, cur = {}, None
    for line in dis.split("\n"):
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            if not m.group(1).startswith("L"):
                cur = kernels.setdefault(m.group(1), [])
            continue
        m = re.match(r"\s+([a-z_0-9]+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):(?:\s+[0-9A-F]{8})+\s*(?:<[^>]*\+0x([0-9a-f]+)>)?", line)
        if m and cur is not None:
            cur.append((int(m.group(3), 16), m.group(1), m.group(2), int(m.group(4), 16) if m.group(4) else None))
    return kernels


def count(ins):
    c = dict.fromkeys(KEYS, 0)
    for _, op, arg, _ in ins:
        c["total"] += 1
        if op.startswith("s_cbranch") or op == "s_branch":
            c["branches"] += 1
            c[op] = c.get(op, 0) + 1
        elif op == "s_waitcnt":
            c["s_waitcnt"] += 1
        elif op == "s_nop":
            c["s_nop"] += 1
        elif op.startswith("s_and_saveexec") or op.startswith("s_or_saveexec"):
            c["s_and_saveexec"] += 1
            c["salu"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
            if op == "s_or_b64" and arg.startswith("exec"):
                c["s_or_exec"] += 1
            if op in ("s_andn2_b64", "s_and_b64", "s_xor_b64", "s_mov_b64") and arg.startswith("exec"):
                c["s_andn2_exec"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            c["vmem"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
    return c


def loops(ins, base):
    """Natural loops [target, backward branch] as index ranges, outermost first."""
    at = {a - base: i for i, (a, _, _, _) in enumerate(ins)}
    out = []
    for i, (a, op, _, tgt) in enumerate(ins):
        if (op.startswith("s_cbranch") or op == "s_branch") and tgt is not None and tgt in at and at[tgt] <= i:
            out.append((at[tgt], i))
    return out


def iteration_loops(ins):
    """The position-iteration loops (<= 32 rows, the wide class, no rows, in program order): a loop body runs the
    serial solves, each under a raised priority (two s_setprio apiece), so it holds four or more s_setprio;
    of the loops that do, the innermost, one per exit branch's target."""
    cand = [(a, b) for a, b in loops(ins, ins[0][0])
            if sum(op == "s_setprio" for _, op, _, _ in ins[a:b]) >= 4]
    inner = [(a, b) for a, b in cand if not any((c, d) != (a, b) and a <= c and d <= b for c, d in cand)]
    out = []
    for a, b in sorted(inner):
        if not out or a > out[-1][1]:
            out.append((a, b))
    # by the rows the loop's sweeps hold, one v_med3_f32 (the row's clamp) each: the <= 32-row class sweeps 16 and
    # 32 rows, the wide class 48 and 63; the free iterations run no sweep. (Not by v_pk_fma_f32: the <= 32-row
    # sweep is the packed one, pgs_sweep_fix, and the wide one, pgs_sweep_tgs, issues scalar FMAs, so the count
    # that was once read as "the wide class issues more" named the two loops the wrong way round.)
    return sorted(out, key=lambda ab: sum(op == "v_med3_f32" for _, op, _, _ in ins[ab[0]:ab[1]]) or 1 << 30)


def main():
    argv = sys.argv[1:]
    extra = argv[argv.index("--") + 1:] if "--" in argv else []
    argv = argv[:argv.index("--")] if "--" in argv else argv
    with tempfile.TemporaryDirectory() as td:
        co = argv[0] if argv else os.path.join(td, "k.co")
        if not argv:
            subprocess.run(B.compile_command("he_physics.hip", extra, device_only=True, out=co), check=True,
                           capture_output=True)
        kernels = disassemble(co)
    ins = next(v for k, v in kernels.items() if re.search(r"\d+physics_kernel_tgsE", k))
    its = iteration_loops(ins)
    cols = [("physics_kernel_tgs", count(ins))]
    for n, (a, b) in enumerate(its):
        cols.append((f"{NAMES[n] if len(its) == 3 else n} [{a}:{b}]", count(ins[a:b + 1])))
    print("%-18s" % "" + "".join("%30s" % name for name, _ in cols))
    for k in KEYS:
        print("%-18s" % k + "".join("%30d" % c[k] for _, c in cols))


if __name__ == "__main__":
    main()
