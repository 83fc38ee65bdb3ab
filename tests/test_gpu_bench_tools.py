"""Every query bench of tools/ (the nine on tools/bench_common.py) run once as a fresh child process at the smallest
size at which all its cases exist: 128 envs (state_bench.py takes two disjoint sets of 64), one warm-up call, two
calls a block, two blocks. Held: exit status 0, and a record with the keys of the committed record at the tool's
default --out, in order, the same cases, finite numbers, and the arguments echoed. No time and no ratio is
asserted: 128 envs measure overheads. Run this file with -x, so that a child that dies stops it.

render_bench.py's record at its default path (profiles/r08) is older than two of the tool's head keys (`cases`,
`render_library`) and than its terrain and ray cases; its head is held to that record's with the two keys where
the tool puts them, its results to profiles/render/terrain_bench.json, the committed record of all its cases."""
import json
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = ["--envs", "128", "--warmup", "1", "--calls", "2", "--blocks", "2"]
ECHO_BLOCKS = dict(envs=128, warmup=1, calls_per_block=2, blocks=2)
TOOLS = {  # tool: (arguments, the record's echo of them, the committed record)
    "dynamics": (["--envs", "128", "--warmup", "1", "--launches", "2", "--repeats", "2"],
                 dict(envs=128, warmup=1, launches=2, repeats=2), "profiles/r09/dynamics_bench.json"),
    "solve": (BLOCKS, ECHO_BLOCKS, "profiles/r12/solve_cost.json"),
    "task": (BLOCKS, ECHO_BLOCKS, "profiles/task/task_bench.json"),
    "centroidal": (BLOCKS, ECHO_BLOCKS, "profiles/centroidal/centroidal_bench.json"),
    "ik": (BLOCKS, ECHO_BLOCKS, "profiles/ik/ik_bench.json"),
    "reaction": (BLOCKS, ECHO_BLOCKS, "profiles/reaction/reaction_bench.json"),
    "derivatives": (BLOCKS + ["--check-envs", "2"], dict(ECHO_BLOCKS, replaced_calls_per_block=1, check_envs=2),
                    "profiles/derivatives/derivatives_bench.json"),
    "state": (BLOCKS, ECHO_BLOCKS, "profiles/state/state_bench.json"),
    "render": (["--warmup", "1", "--launches", "2"], dict(warmup=1, launches=2), "profiles/r08/render_bench.json"),
}


def _numbers(x):
    if isinstance(x, dict):
        x = list(x.values())
    if isinstance(x, list):
        for y in x:
            yield from _numbers(y)
    elif isinstance(x, (int, float)) and not isinstance(x, bool):
        yield x


@pytest.mark.parametrize("tool", list(TOOLS))
def test_bench_tool(tool, tmp_path):
    argv, echo, committed = TOOLS[tool]
    out = tmp_path / "record.json"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool + "_bench.py"), "--out", str(out)] + argv,
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    rec = json.loads(out.read_text())
    ref = json.load(open(os.path.join(ROOT, committed)))
    head, results = list(ref), ref["results"]
    if tool == "render":
        at = head.index("primitives_per_env") + 1
        head[at:at] = ["cases", "render_library"]
        results = json.load(open(os.path.join(ROOT, "profiles", "render", "terrain_bench.json")))["results"]
    assert list(rec) == head
    assert [r["case"] for r in rec["results"]] == [r["case"] for r in results]
    for new, old in zip(rec["results"], results):
        assert list(new) == list(old), new["case"]
        for key, value in new.items():
            if key.endswith("_blocks_ms") or key == "ms_repeats":
                assert len(value) == 2, (new["case"], key)
    assert {k: rec[k] for k in echo} == echo
    numbers = list(_numbers(rec))
    assert len(numbers) > len(rec["results"]) and all(math.isfinite(v) for v in numbers)
