"""CPU checks of the external-wrench interface (he_apply_body_forces, he_apply_body_forces_at_pos;
gym.apply_rigid_body_force_tensors, puffer_phc/envs/render_env.py:105-126): the header with the new
prototypes compiles as C, the ctypes prototypes and the space constants exist with the header's
values, and the env's push option is off by default. The GPU side is tests/test_gpu_body_forces.py."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_with_wrench_prototypes_compiles_as_c(tmp_path):
    src = tmp_path / "f.c"
    src.write_text('#include <stdio.h>\n#include "humanoid_engine.h"\n'
                   "int main(void){\n"
                   "  int (*a)(he_engine*, const float*, const float*, int, int, void*) = he_apply_body_forces;\n"
                   "  int (*b)(he_engine*, const float*, const float*, int, int, void*) = he_apply_body_forces_at_pos;\n"
                   '  printf("%d %d %d %d %d\\n", HE_SPACE_ENV, HE_SPACE_LOCAL, HE_SPACE_GLOBAL, (int)HE_BUF_COUNT, a != b);\n'
                   "  return 0;}\n")
    obj = tmp_path / "f.o"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)],
                   check=True)
    # the values through the preprocessor (no engine library is linked)
    pre = tmp_path / "v.c"
    pre.write_text('#include <stdio.h>\n#include "humanoid_engine.h"\n'
                   'int main(void){printf("%d %d %d %d\\n", HE_SPACE_ENV, HE_SPACE_LOCAL, HE_SPACE_GLOBAL, (int)HE_BUF_COUNT);return 0;}\n')
    exe = tmp_path / "v"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(pre), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [0, 1, 2, 12]  # no buffer kind was added


def test_abi_prototypes_and_space_constants():
    from humanoid_amd import _abi, engine
    from humanoid_amd.isaacgym import gymapi
    assert (_abi.SPACE_ENV, _abi.SPACE_LOCAL, _abi.SPACE_GLOBAL) == (0, 1, 2)
    assert (gymapi.ENV_SPACE, gymapi.LOCAL_SPACE, gymapi.GLOBAL_SPACE) == (0, 1, 2)
    want = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    assert _abi.FORCE_PROTOTYPES == {"he_apply_body_forces": want, "he_apply_body_forces_at_pos": want}
    assert set(_abi.FORCE_PROTOTYPES) <= set(engine.HE_SYMBOLS)
    lib = engine.load_library()  # loads without a GPU
    for name in _abi.FORCE_PROTOTYPES:
        fn = getattr(lib, name)
        assert fn.argtypes == want and fn.restype is C.c_int
    for name in ("apply_body_forces", "apply_body_forces_at_pos", "clear_body_forces"):
        assert callable(getattr(engine.Engine, name))
    for name in ("apply_rigid_body_force_tensors", "apply_rigid_body_force_at_pos_tensors"):
        assert callable(getattr(gymapi.Gym, name))


def test_invalid_calls_are_refused_without_gpu():
    """A null handle is an error with a reason, whatever else is passed."""
    from humanoid_amd import engine
    lib = engine.load_library()
    for fn in (lib.he_apply_body_forces, lib.he_apply_body_forces_at_pos):
        assert fn(None, None, None, 0, 1, None) != 0
        assert b"null handle" in lib.he_last_error()


def test_env_config_has_pushes_off():
    from humanoid_amd.env import EnvConfig
    c = EnvConfig()
    assert (c.push_interval, c.push_duration, c.push_force, c.push_body, c.push_in_eval) == (0, 2, 0.0, "Torso", False)
