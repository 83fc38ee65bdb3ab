"""Diagnostics: build the engine library with extra -D flags on the physics TU into
humanoid_amd/_variants/<name>.so, for A/B timing on one GPU box (HE_ENGINE_LIB=<path>).
Usage: python tools/build_variant.py NAME [--tu he_imitation.hip] [-DFOO=1 ...] [-mllvm -opt ...]
(an -amdgpu-sched-strategy= given here replaces the product's max-ilp)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from humanoid_amd import build as B  # noqa: E402


OUT_DIR = os.path.join(ROOT, "humanoid_amd", "_variants")


def variant_command(name, tu, defs):
    """The variant object's compile line (the product's, humanoid_amd.build.compile_command, with defs) and its path."""
    obj = os.path.join(OUT_DIR, name + "." + tu + ".o")
    cmd = B.compile_command(tu, defs, out=obj)
    if any(d.startswith("-amdgpu-sched-strategy=") for d in defs) and "-amdgpu-sched-strategy=max-ilp" in dict(B.SOURCES)[tu]:
        i = cmd.index("-amdgpu-sched-strategy=max-ilp")  # a variant's strategy replaces the product's (the first)
        del cmd[i - 1:i + 1]
    return cmd, obj


def main():
    name, defs = sys.argv[1], sys.argv[2:]
    tu = "he_physics.hip"
    if defs[:1] == ["--tu"]:
        tu, defs = defs[1], defs[2:]
    B.build()
    out_dir = OUT_DIR
    os.makedirs(out_dir, exist_ok=True)
    cmd, obj = variant_command(name, tu, defs)
    subprocess.run(cmd, check=True)
    objs = [obj if src == tu else os.path.join(B.BUILD, src + ".o") for src, _ in B.SOURCES]
    lib = os.path.join(out_dir, name + ".so")
    subprocess.run([B._hipcc(), "--offload-arch=" + B.ARCH, "-shared", "-fPIC", "-o", lib] + objs, check=True)
    print(lib)


if __name__ == "__main__":
    main()
