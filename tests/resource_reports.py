"""Synthetic kernel-resource-usage remarks in the compiler's words (tests/data/he_physics_resource_report.txt
is a real report), for the tests of humanoid_amd.build.check_resources: a kernel is named as the source writes
it ("physics_kernel", "render_kernel<false>") and printed under the symbol the compiler gives it."""
from humanoid_amd import build

# (the report's line, its keyword here, the figure printed when none is given); None leaves the line out
LINES = (("VGPRs", "vgprs", 128), ("ScratchSize [bytes/lane]", "scratch", 0), ("Occupancy [waves/SIMD]", "occupancy", 2),
         ("SGPRs Spill", "spilled_sgprs", 0), ("VGPRs Spill", "spilled_vgprs", 0))


def symbol(kernel):
    """The anonymous-namespace Itanium symbol of void kernel(Params), a template's with its bool arguments:
    render_kernel<false> is _ZN12_GLOBAL__N_113render_kernelILb0EEEvNS_6ParamsE."""
    name, _, args = kernel.partition("<")
    args = "".join({"false": "Lb0E", "true": "Lb1E"}[a.strip()] for a in args.rstrip(">").split(",")) if args else ""
    return f"_ZN12_GLOBAL__N_1{len(name)}{name}" + (f"I{args}EEv" if args else "E") + "NS_6ParamsE"


def block(kernel, **figures):
    lines = [f"Function Name: {symbol(kernel)}"] + [f"    {label}: {figures.get(key, default)}"
                                                    for label, key, default in LINES if figures.get(key, default) is not None]
    return "".join(f"k.hip:1:1: remark: {ln} [-Rpass-analysis=kernel-resource-usage]\n" for ln in lines)


def report(kernels):
    """{kernel: its figures by LINES' keywords} as one report, the blocks in the dict's order."""
    return "".join(block(k, **figures) for k, figures in kernels.items())


def at_budget(src, changes=None, order=None, without=()):
    """The report of a checked source with every kernel exactly at its budget (a figure that is not held:
    LINES' default). changes: {kernel: figures} laid over that; order: the blocks' order (default: the
    table's); without: kernels whose blocks are left out."""
    kernels = {}
    for name in order or build.BUDGETS[src]:
        b = build.BUDGETS[src][name]
        held = {"occupancy": b.min_waves, "scratch": b.max_scratch, "spilled_vgprs": b.max_spilled_vgprs}
        kernels[name] = {k: v for k, v in held.items() if v is not None} | (changes or {}).get(name, {})
    return report({k: f for k, f in kernels.items() if k not in without})
