"""CPU checks of the build's resource gate (humanoid_amd.build: BUDGETS, kernel_name, check_resources) on the
compiler's own words: a committed report of he_physics.hip, a live compile of hd_dynamics.hip, and synthetic
reports (tests/resource_reports.py) for exact names, template arguments, unlisted functions and the twin.
The failure modes by source are in test_abi.py, test_solve.py and test_centroidal.py."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

from humanoid_amd import build
from resource_reports import at_budget, report, symbol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# hipcc's remarks for he_physics.hip, device only: compile_command("he_physics.hip", [build.REPORT_FLAG],
# device_only=True, out=...), the remark lines with the source's directory cut off
PHYSICS_REPORT = os.path.join(ROOT, "tests", "data", "he_physics_resource_report.txt")
# kernel: (waves/SIMD, scratch bytes/lane, spilled VGPRs)
PHYSICS_FIGURES = {"physics_kernel": (2, 0, 0), "physics_kernel_tgs": (2, 148, 36), "physics_kernel_ext": (2, 0, 0),
                   "physics_kernel_tgs_ext": (2, 156, 38), "physics_order_kernel": (8, 0, 0), "warm_tu_kernel": (8, 0, 0)}


def test_kernel_names_are_exact():
    assert build.kernel_name("_ZN12_GLOBAL__N_114physics_kernelE8PhysArgs") == "physics_kernel"
    assert build.kernel_name("_ZN12_GLOBAL__N_122physics_kernel_tgs_extE8PhysArgs") == "physics_kernel_tgs_ext"
    assert build.kernel_name("_ZN12_GLOBAL__N_120physics_order_kernelEPKjPii") == "physics_order_kernel"
    assert build.kernel_name("_ZN12_GLOBAL__N_114warm_tu_kernelEv") == "warm_tu_kernel"
    assert build.kernel_name("_ZN12_GLOBAL__N_113render_kernelILb0EEEvNS_6ParamsE") == "render_kernel<false>"
    assert build.kernel_name("_ZN12_GLOBAL__N_113render_kernelILb1EEEvNS_6ParamsE") == "render_kernel<true>"
    assert build.kernel_name("_ZN12_GLOBAL__N_11kILb1ELi3ELin2EEEvv") == "k<true, 3, -2>"
    assert build.kernel_name("physics_kernel") == "physics_kernel"  # a bare name as it is
    # template arguments that are no literals keep their mangling: such a name matches no entry
    assert build.kernel_name("_ZN12_GLOBAL__N_11kIfEEvv") not in ("k", "k<>")
    for kernels in build.BUDGETS.values():  # the helper's symbols are the compiler's
        for k in kernels:
            assert build.kernel_name(symbol(k)) == k


def test_committed_physics_report():
    text = open(PHYSICS_REPORT).read()
    assert "/" not in text.replace("[waves/SIMD]", "").replace("[bytes/lane]", "").replace("[bytes/block]", "")
    blocks = build.kernel_reports(text)
    assert {k: (b["occupancy"], b["scratch"], b["spilled_vgprs"]) for k, b in blocks.items()} == PHYSICS_FIGURES
    assert blocks["physics_kernel_tgs"]["fields"]["VGPRs"] == "256"  # resource_report's shape, as tools/spill_map.py reads it
    assert set(build.resource_report(text)) == {
        "_ZN12_GLOBAL__N_114physics_kernelE8PhysArgs", "_ZN12_GLOBAL__N_118physics_kernel_tgsE8PhysArgs",
        "_ZN12_GLOBAL__N_118physics_kernel_extE8PhysArgs", "_ZN12_GLOBAL__N_122physics_kernel_tgs_extE8PhysArgs",
        "_ZN12_GLOBAL__N_120physics_order_kernelEPKjPii", "_ZN12_GLOBAL__N_114warm_tu_kernelEv"}
    build.check_resources("he_physics.hip", text, product=True)
    build.check_resources("he_physics.hip", text, product=False)
    # the EXT kernel's scratch alone, one byte up: it fails, and names that kernel and no other
    line = "he_physics.hip:405:1: remark:     ScratchSize [bytes/lane]: 156 "
    assert text.count(line) == 1
    with pytest.raises(RuntimeError) as e:
        build.check_resources("he_physics.hip", text.replace(line, line.replace("156", "157")))
    assert str(e.value).startswith("physics_kernel_tgs_ext: 157 bytes/lane of scratch, 38 spilled VGPRs; the ceiling is 156 / 38")
    assert not [k for k in PHYSICS_FIGURES if k != "physics_kernel_tgs_ext" and re.search(rf"\b{k}\b", str(e.value))]


def test_live_report_of_the_dynamics_source(tmp_path):
    if shutil.which(build._hipcc()) is None:
        pytest.skip("hipcc not present")
    cmd = build.compile_command("hd_dynamics.hip", [build.REPORT_FLAG], device_only=True, out=str(tmp_path / "k.co"))
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    build.check_resources("hd_dynamics.hip", r.stderr)
    blocks = build.kernel_reports(r.stderr)
    assert set(blocks) == {"dynamics_kernel", "centroidal_kernel"}
    assert all(b["scratch"] == 0 and b["occupancy"] is not None and b["spilled_vgprs"] is not None for b in blocks.values())


def test_a_function_outside_the_table_fails_and_is_named():
    for src, extra in (("he_physics.hip", "physics_kernel_new"), ("hd_dynamics.hip", "centroidal_kernel<true>"),
                       ("hr_render.hip", "render_kernel"), ("ht_task.hip", "task_kernel_ext")):
        text = at_budget(src) + report({extra: {}})
        for product in (True, False):
            with pytest.raises(RuntimeError, match=re.escape(f"{extra}: a function of {src} that build.BUDGETS does not name")):
                build.check_resources(src, text, product)
    # and a kernel deleted from the table is such a function
    kept = dict(build.BUDGETS["hr_render.hip"])
    try:
        del build.BUDGETS["hr_render.hip"]["rays_kernel"]
        with pytest.raises(RuntimeError, match="rays_kernel: a function of hr_render.hip"):
            build.check_resources("hr_render.hip", report(dict.fromkeys(kept, {})))
    finally:
        build.BUDGETS["hr_render.hip"] = kept
    build.check_resources("hr_render.hip", report(dict.fromkeys(kept, {})))
    # a source without entries may hold anything
    build.check_resources("he_ingest.hip", report({"ingest_kernel": {"scratch": 64, "occupancy": 1}}))


def test_each_physics_kernel_reads_its_own_block():
    """The four physics kernels' names are prefixes of one another: under every order of their blocks, a
    figure over the ceiling in one kernel's block fails under that kernel's name, and in no other order passes."""
    four = ["physics_kernel", "physics_kernel_ext", "physics_kernel_tgs", "physics_kernel_tgs_ext"]
    rest = [k for k in build.BUDGETS["he_physics.hip"] if k not in four]
    for order in itertools.permutations(four):
        build.check_resources("he_physics.hip", at_budget("he_physics.hip", order=list(order) + rest))
        for k in four:
            _, b, v = build.BUDGETS["he_physics.hip"][k]
            with pytest.raises(RuntimeError) as e:
                build.check_resources("he_physics.hip", at_budget("he_physics.hip", {k: {"scratch": b + 4}}, order=rest + list(order)))
            assert str(e.value).startswith(f"{k}: {b + 4} bytes/lane of scratch, {v} spilled VGPRs; the ceiling is {b} / {v} ")
            with pytest.raises(RuntimeError, match=rf"^{k}: occupancy 1 waves/SIMD < 2 "):
                build.check_resources("he_physics.hip", at_budget("he_physics.hip", {k: {"occupancy": 1}}, order=list(order) + rest))


def test_template_instantiations_are_told_apart():
    for bad, good in (("render_kernel<false>", "render_kernel<true>"), ("render_kernel<true>", "render_kernel<false>")):
        for order in ((bad, good, "rays_kernel"), ("rays_kernel", good, bad)):
            with pytest.raises(RuntimeError, match=f"^{bad}: 16 bytes/lane of scratch"):
                build.check_resources("hr_render.hip", at_budget("hr_render.hip", {bad: {"scratch": 16}}, order=order))
        with pytest.raises(RuntimeError, match=f"^{bad}: not in the compiler's resource report"):
            build.check_resources("hr_render.hip", at_budget("hr_render.hip", without=[bad]))


def test_the_twin_is_held_to_occupancy_alone():
    over = {"physics_kernel_tgs": {"scratch": 148, "spilled_vgprs": 44}, "physics_kernel": {"scratch": 8, "spilled_vgprs": 2}}
    build.check_resources("he_physics.hip", at_budget("he_physics.hip", over), product=False)
    with pytest.raises(RuntimeError, match="^physics_kernel: 8 bytes/lane of scratch, 2 spilled VGPRs"):
        build.check_resources("he_physics.hip", at_budget("he_physics.hip", over), product=True)
    # its missing spill lines are not read either; its occupancy is, and so is the list of its kernels
    cut = {k: {"scratch": None, "spilled_vgprs": None} for k in build.BUDGETS["he_physics.hip"]}
    build.check_resources("he_physics.hip", at_budget("he_physics.hip", cut), product=False)
    with pytest.raises(RuntimeError, match="^physics_kernel_ext: occupancy 1 waves/SIMD < 2"):
        build.check_resources("he_physics.hip", at_budget("he_physics.hip", over | {"physics_kernel_ext": {"occupancy": 1}}), product=False)
    with pytest.raises(RuntimeError, match="^physics_kernel_ext: not in the compiler's resource report"):
        build.check_resources("he_physics.hip", at_budget("he_physics.hip", without=["physics_kernel_ext"]), product=False)
