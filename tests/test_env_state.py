"""CPU checks of the env-state calls (include/humanoid_engine.h "env state": he_state_layout_get, he_save_envs,
he_load_envs, he_clone_envs, he_get_sim_state, he_set_sim_state): the header as C99, the structs against their
ctypes mirrors, the exported symbols, the refusals in the header's order, the layout out of the buffer table, the
binding's argument checks, and HumanoidPHC.save_state through torch.save.

A refusal that a handle must get past its null check is sent with a stand-in handle, a zeroed block of memory:
every call checks its arguments before it reads more of the handle than its env count, and a zeroed handle is
one without envs. The refusals behind "no envs created" need a live engine: tests/test_gpu_env_state.py."""
import ctypes as C
import io
import os
import subprocess

import pytest

from humanoid_amd import _abi

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("he_state_layout_get", "he_save_envs", "he_load_envs", "he_clone_envs", "he_get_sim_state",
           "he_set_sim_state")
# the included rows in table order, in words per env (include/humanoid_engine.h he_buf_kind): root 13,
# dof state 69 x 2, rigid bodies 24 x 13, contact forces 24 x 3, dof forces 69, targets 69, the two counts,
# the cache 104, the initial root 13, then the wrench rows 24 x 6 and the actuation row 69
FIELDS = (("root", 0, 13, 1), ("dof_state", 1, 138, 1), ("rb", 2, 312, 1), ("cf", 3, 72, 1), ("dof_force", 4, 69, 1),
          ("targets", 5, 69, 1), ("num_contacts", 6, 1, 2), ("dropped", 7, 1, 2), ("cache", 8, 104, 1),
          ("init_root", 9, 13, 1), ("wrench", -1, 144, 1), ("dof_act", -1, 69, 1))


def _lib():
    from humanoid_amd import engine
    return engine.load_library()


def test_header_compiles_as_c99_and_structs_match_ctypes(tmp_path):
    src = tmp_path / "state.c"
    names = (("he_state_field", ("kind", "offset_words", "words", "dtype")),
             ("he_state_layout", ("version", "words", "num_fields", "fields")),
             ("he_sim_state", ("version", "wrench_hold", "act_set", "launches")))
    prints = "".join(f'printf("%zu", sizeof({s}));' + "".join(f'printf(" %zu", offsetof({s}, {m}));' for m in ms)
                     + 'printf("\\n");' for s, ms in names)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "humanoid_engine.h"\n'
                   f'int main(void){{{prints}printf("%d %d\\n", HE_STATE_VERSION, HE_STATE_MAX_FIELDS);return 0;}}\n')
    exe = tmp_path / "state"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, (cls, (_, members)) in zip(out, zip((_abi.HeStateField, _abi.HeStateLayout, _abi.HeSimState), names)):
        want = [C.sizeof(cls)] + [getattr(cls, m).offset for m in members]
        assert [int(x) for x in line.split()] == want, cls.__name__
    assert [int(x) for x in out[3].split()] == [_abi.STATE_VERSION, _abi.STATE_MAX_FIELDS]


def test_symbols_are_exported_and_bound():
    from humanoid_amd import engine
    lib = C.CDLL(engine.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in engine.HE_SYMBOLS and engine.HE_PROTOTYPES[s] is _abi.STATE_PROTOTYPES[s]
    assert tuple(_abi.STATE_PROTOTYPES) == SYMBOLS
    lib.he_version.restype = C.c_int
    assert lib.he_version() == 1


def test_layout_follows_the_buffer_table():
    """The layout is host-only and needs no envs: a zeroed stand-in handle gives it. Fields are contiguous
    and in table order; PHYS_ORDER (10), PHYS_COST (11) and the metadata cache (a third internal row) are absent."""
    lib = _lib()
    block = C.create_string_buffer(1 << 16)
    layout = _abi.HeStateLayout()
    assert lib.he_state_layout_get(C.cast(block, C.c_void_p), C.byref(layout)) == 0
    assert block.raw == bytes(1 << 16)
    assert layout.version == _abi.STATE_VERSION and layout.num_fields == len(FIELDS) <= _abi.STATE_MAX_FIELDS
    offset = 0
    for f, (_, kind, words, dtype) in zip(layout.fields, FIELDS):
        assert (f.kind, f.offset_words, f.words, f.dtype) == (kind, offset, words, dtype)
        offset += words
    assert layout.words == offset == 1005
    kinds = [f.kind for f in layout.fields[:layout.num_fields]]
    assert _abi.BUF_PHYS_ORDER not in kinds and _abi.BUF_PHYS_COST not in kinds and kinds.count(-1) == 2
    words, fields = _abi.state_fields(layout)
    assert words == 1005 and list(fields) == [name for name, *_ in FIELDS]
    assert fields["cache"] == (675, 104, _abi.DTYPE_F32) and fields["num_contacts"] == (673, 1, _abi.DTYPE_I32)


def test_refusals_come_in_the_stated_order():
    lib = _lib()

    def reason(rc):
        assert rc != 0
        return lib.he_last_error().decode()

    block = C.create_string_buffer(1 << 16)
    fake = C.cast(block, C.c_void_p)
    odd = C.c_void_p(8194)
    bad_sim = _abi.HeSimState(version=7, wrench_hold=-1, act_set=0, launches=-1)
    # 1, the null handle, with everything after it wrong as well: no pointer, k out of range, odd addresses
    assert "he_save_envs: null handle" in reason(lib.he_save_envs(None, odd, -1, None, None))
    assert "he_load_envs: null handle" in reason(lib.he_load_envs(None, odd, -1, None, None))
    assert "he_clone_envs: null handle" in reason(lib.he_clone_envs(None, None, odd, -1, None))
    assert "he_state_layout_get: null handle" in reason(lib.he_state_layout_get(None, None))
    assert "he_get_sim_state: null handle" in reason(lib.he_get_sim_state(None, None))
    assert "he_set_sim_state: null handle" in reason(lib.he_set_sim_state(None, C.byref(bad_sim)))
    # 2, no envs, likewise
    assert "he_save_envs: no envs created" in reason(lib.he_save_envs(fake, odd, -1, None, None))
    assert "he_load_envs: no envs created" in reason(lib.he_load_envs(fake, odd, 1 << 30, None, None))
    assert "he_clone_envs: no envs created" in reason(lib.he_clone_envs(fake, None, odd, -1, None))
    assert "he_get_sim_state: no envs created" in reason(lib.he_get_sim_state(fake, None))
    assert "he_set_sim_state: no envs created" in reason(lib.he_set_sim_state(fake, C.byref(bad_sim)))
    assert "he_set_sim_state: no envs created" in reason(lib.he_set_sim_state(fake, None))
    # the layout needs no envs; its second refusal is the null output
    assert "he_state_layout_get: null layout" in reason(lib.he_state_layout_get(fake, None))
    assert block.raw == bytes(1 << 16)  # the stand-in handle was never written


class _NoCalls:
    """Stands in for the library: any call is a failure of the check under test."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the argument check")


def _unbound(n=3):
    from humanoid_amd.engine import Engine
    o = object.__new__(Engine)
    o.lib, o.h, o.device, o.num_envs = _NoCalls(), None, torch.device("cpu"), n
    offset, fields = 0, {}
    for name, _, words, dtype in FIELDS:
        fields[name] = (offset, words, dtype)
        offset += words
    o._state_layout = (offset, fields)
    return o


def test_engine_argument_checks_raise_before_any_library_call():
    from humanoid_amd.engine import EngineError
    o = _unbound()
    w = o.state_layout[0]
    ids = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(EngineError, match="save_envs ids"):
        o.save_envs(ids=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(EngineError, match="save_envs ids"):
        o.save_envs(ids=torch.zeros(4, dtype=torch.int32))  # more ids than envs
    with pytest.raises(EngineError, match="save_envs ids"):
        o.save_envs(ids=torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(EngineError, match="save_envs ids"):
        o.save_envs(ids=[0, 1])
    with pytest.raises(EngineError, match="save_envs out"):
        o.save_envs(ids=ids, out=torch.zeros(3, w, dtype=torch.int32))  # k rows, not num_envs
    with pytest.raises(EngineError, match="save_envs out"):
        o.save_envs(out=torch.zeros(3, w, dtype=torch.float32))
    with pytest.raises(EngineError, match="save_envs out"):
        o.save_envs(out=torch.zeros(w, 3, dtype=torch.int32).t())
    with pytest.raises(EngineError, match="load_envs state"):
        o.load_envs(torch.zeros(3, w - 1, dtype=torch.int32))
    with pytest.raises(EngineError, match="load_envs state"):
        o.load_envs(torch.zeros(3, w, dtype=torch.int32), ids=ids)
    with pytest.raises(EngineError, match="load_envs ids"):
        o.load_envs(torch.zeros(2, w, dtype=torch.int32), ids=ids.float())
    with pytest.raises(EngineError, match="both required"):
        o.clone_envs(ids, None)
    with pytest.raises(EngineError, match="clone_envs dst_ids"):
        o.clone_envs(ids, ids.long())
    with pytest.raises(EngineError, match="2 sources for 1 destinations"):
        o.clone_envs(ids, ids[:1])
    with pytest.raises(EngineError, match="no field 'order'"):
        o.state_field(torch.zeros(2, w, dtype=torch.int32), "order")
    with pytest.raises(EngineError, match="packed states"):
        o.state_field(torch.zeros(2, w, dtype=torch.float32), "root")
    # the typed views share the tensor's memory
    s = torch.arange(2 * w, dtype=torch.int32).reshape(2, w)
    root, count = o.state_field(s, "root"), o.state_field(s, "num_contacts")
    assert root.dtype == torch.float32 and root.shape == (2, 13) and root.data_ptr() == s.data_ptr()
    assert count.dtype == torch.int32 and count.tolist() == [[673], [w + 673]]
    root[1, 0] = 1.0
    assert s[1, 0].item() == 0x3F800000


def _stub_env(n=3, amp=False):
    """A HumanoidPHC with host tensors and a stand-in engine: what save_state reads, and no more."""
    from humanoid_amd.env import EnvConfig, HumanoidPHC
    g = torch.Generator().manual_seed(5)
    e = object.__new__(HumanoidPHC)
    e.cfg = EnvConfig(num_envs=n, use_amp_obs=amp)
    e.device = torch.device("cpu")
    e.flag_test = e.flag_im_eval = False
    e.obs_buf, e.rew_buf, e.reward_raw = torch.rand(n, 934, generator=g), torch.rand(n, generator=g), torch.rand(n, 5, generator=g)
    e.progress_buf = torch.arange(n, dtype=torch.int16)
    e._reset_u8, e._term_u8 = torch.ones(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8)
    e._global_offset, e._motion_start_times = torch.rand(n, 3, generator=g), torch.rand(n, generator=g)
    e._motion_start_times_offset, e._sampled_motion_ids = torch.zeros(n), torch.arange(n)
    e._motion_sample_start_idx, e._push_step, e._push_left, e._push_f = 6, 9, 1, torch.rand(n, 24, 3, generator=g)
    if amp:
        e._amp_obs_buf, e._amp_obs_demo_buf = torch.rand(n, 10, 196, generator=g), torch.rand(n, 10, 196, generator=g)
    e._gen = torch.Generator().manual_seed(11)
    torch.rand(3, generator=e._gen)
    e._push_gen = torch.Generator().manual_seed(12)  # the noise generator has not drawn: absent

    class Lib:
        _curr_motion_ids, _sampling_prob, _termination_history = torch.arange(n), torch.ones(4) / 4, torch.zeros(4)
        _gen = torch.Generator().manual_seed(13)

    class Eng:
        def save_envs(self):
            return torch.arange(n * 1005, dtype=torch.int32).reshape(n, 1005)

        def sim_state_dict(self):
            return {"version": 1, "wrench_hold": 3, "act_set": 1, "launches": 40}

    e._motion_lib, e.engine = Lib(), Eng()
    return e


@pytest.mark.parametrize("amp", [False, True])
def test_save_state_round_trips_through_torch_save(amp):
    e = _stub_env(amp=amp)
    d = e.save_state()
    for name in ("engine", "sim_state", "progress_buf", "_sampled_motion_ids", "_motion_start_times",
                 "_motion_start_times_offset", "_global_offset", "motion_sample_start_idx", "_reset_u8", "_term_u8",
                 "obs_buf", "rew_buf", "reward_raw", "push_step", "push_left", "push_f", "generator_gen",
                 "generator_noise_gen", "generator_push_gen", "loaded_motion_ids"):
        assert name in d, name
    assert ("_amp_obs_buf" in d) == ("_amp_obs_demo_buf" in d) == amp
    assert d["generator_noise_gen"] is None and d["generator_gen"].dtype == torch.uint8
    assert torch.equal(d["generator_gen"], e._gen.get_state())
    # copies, not views: a later step does not move a saved state
    assert d["obs_buf"].data_ptr() != e.obs_buf.data_ptr() and torch.equal(d["obs_buf"], e.obs_buf)
    f = io.BytesIO()
    torch.save(d, f)
    f.seek(0)
    back = torch.load(f)
    assert back.keys() == d.keys()
    for k, v in d.items():
        if isinstance(v, torch.Tensor):
            assert back[k].dtype == v.dtype and torch.equal(back[k], v), k
        else:
            assert back[k] == v and type(back[k]) is type(v), k
