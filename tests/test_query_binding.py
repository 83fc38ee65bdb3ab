"""CPU checks of what the three query bindings (humanoid_amd/dynamics.py, solve.py, task.py) share through
humanoid_amd/_abi.py: one base class, one statement of the flags, each module's own error class on a
refused state tensor, and the names each module has always exported. The objects are unbound (no
library, no engine, no GPU); the calls themselves are checked in each library's own tests."""
import pytest

from humanoid_amd import _abi, dynamics, solve, task

BINDINGS = [(dynamics, dynamics.Dynamics, dynamics.DynamicsError, "hd", "HD"),
            (solve, solve.Solver, solve.SolveError, "hs", "HS"),
            (task, task.TaskSpace, task.TaskError, "ht", "HT")]
IDS = [m.__name__.rsplit(".", 1)[1] for m, *_ in BINDINGS]


class _NoCalls:
    """Stands in for the library: any call is a failure of the check under test."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the argument check")


def _unbound(cls, engine=None):
    import torch
    o = object.__new__(cls)
    o.lib, o.h, o.engine = _NoCalls(), None, engine
    o.device, o.num_envs, o.armature, o.gravity = torch.device("cuda", 0), 3, True, True
    return o


@pytest.mark.parametrize("module,cls,error,prefix,upper", BINDINGS, ids=IDS)
def test_class_derives_from_the_one_base(module, cls, error, prefix, upper):
    assert issubclass(cls, _abi.QueryBinding) and cls is not _abi.QueryBinding
    # the constructor, the destructor and the helpers are the base's: stated once
    for name in ("__del__", "flags", "_flags", "_states", "_out"):
        assert name not in vars(cls) and hasattr(cls, name), name
    assert cls.LIBRARY.prefix == prefix and cls.LIBRARY.error_cls is error and cls.LIBRARY.path == module.LIB_PATH
    assert cls.LIBRARY.prototypes is getattr(module, upper + "_PROTOTYPES")
    assert cls.NO_CPU_PATH.endswith("no CPU path")


@pytest.mark.parametrize("module,cls,error,prefix,upper", BINDINGS, ids=IDS)
def test_flags_follow_armature_and_gravity(module, cls, error, prefix, upper):
    o = _unbound(cls)
    for armature in (False, True):
        for gravity in (False, True):
            o.armature, o.gravity = armature, gravity
            want = (module.FLAG_ARMATURE if armature else 0) | (0 if gravity else module.FLAG_NO_GRAVITY)
            assert o.flags == want == o._flags(None)
    assert o._flags(2) == 2
    assert (module.FLAG_ARMATURE, module.FLAG_NO_GRAVITY, module.FLAGS_DEFAULT) == (1, 2, 1)


@pytest.mark.parametrize("module,cls,error,prefix,upper", BINDINGS, ids=IDS)
def test_wrong_device_root_state_raises_the_modules_own_error(module, cls, error, prefix, upper):
    """A root_state on the CPU is refused with the module's error class, by name, before any library call
    (and before the engine is read: it is None here)."""
    import torch
    o = _unbound(cls)
    others = [e for _, _, e, _, _ in BINDINGS if e is not error]
    with pytest.raises(error, match="root_state") as e:
        o._states(torch.zeros(3, 13), torch.zeros(3 * _abi.ND, 2))
    assert not isinstance(e.value, tuple(others))
    with pytest.raises(error, match="out"):
        o._out(torch.zeros(3, 75), (3, 75), "out")


@pytest.mark.parametrize("module,cls,error,prefix,upper", BINDINGS, ids=IDS)
def test_module_still_exports_its_names(module, cls, error, prefix, upper):
    for name in ("LIB_PATH", "load_library", "validate_model", "check_tensor", upper + "_PROTOTYPES", upper + "_SYMBOLS",
                 "FLAG_ARMATURE", "FLAG_NO_GRAVITY", "FLAGS_DEFAULT", "NG"):
        assert hasattr(module, name), name
    assert module.NG == _abi.NG == 75
    assert getattr(module, upper + "_SYMBOLS") == tuple(getattr(module, upper + "_PROTOTYPES"))
    assert module.LIB_PATH.endswith(f"libhumanoid_{module.__name__.rsplit('.', 1)[1]}.so")
    assert all(callable(getattr(module, f)) for f in ("load_library", "validate_model", "check_tensor"))
    assert issubclass(error, RuntimeError) and error.__module__ == module.__name__
    # the module's check_tensor raises the module's error
    with pytest.raises(error, match="x: expected a torch tensor"):
        module.check_tensor(None, None, (1,), None, "x")


def test_each_modules_own_constants_stay():
    assert solve.MAX_RHS == 32 and task.MAX_ROWS == 32 and dynamics.JAC_ROWS == 6
    assert task.MODES == {"force": 0, "joint": 1} and len(task.TERMS) == 5
    assert callable(task.make_rows) and task.HtRow._fields_[0][0] == "body"
    assert isinstance(dynamics.Dynamics.solver, property) and isinstance(dynamics.Dynamics.task, property)
