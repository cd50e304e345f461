"""Densification without a GPU: the entry points are exported and bound, every argument error is reported by the host
before any launch, and the Python layer refuses bad arguments before it touches the device."""
import ctypes
import importlib

import pytest
import torch

import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import _native
from taichi_gaussian_rasterizer_amd.optim import ParameterClass

# the package exports the function `densify`, which hides the module of that name as an attribute
dn = importlib.import_module("taichi_gaussian_rasterizer_amd.densify")
ENTRY_POINTS = ("gs_densify_plan_scratch_bytes", "gs_densify_plan", "gs_table_move_rows", "gs_split3d_children",
                "gs_densify_accumulate")
FAKE = 0x10000  # a non-NULL, 16-byte aligned address: validation fails before anything could read it


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.lib()


def err(lib):
    return lib.gs_last_error()


def test_exports_and_bindings(lib):
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(handle, name), name
        assert name in _native.SIGNATURES, name
    for name in ("DensifyPlan", "DensifyStats", "densify", "move_rows", "plan_densify", "split_gaussians3d"):
        assert name in gs.__all__ and getattr(gs, name) is getattr(dn, name), name
    assert ctypes.sizeof(_native.GsMoveColumn) == 32
    assert _native.GsMoveColumn.copy_rows.offset == 24 and _native.GsMoveColumn.row_bytes.offset == 16
    assert (_native.GS_MOVE_COLUMNS_MAX, _native.GS_DENSIFY_CHILDREN_MAX, _native.GS_DENSIFY_STATS) == (32, 8, 6)


def test_plan_scratch_size(lib):
    assert lib.gs_densify_plan_scratch_bytes(0) == 0 and lib.gs_densify_plan_scratch_bytes(-3) == 0
    small, large = lib.gs_densify_plan_scratch_bytes(1), lib.gs_densify_plan_scratch_bytes(10_000_000)
    assert small >= 2 * 4 * 4 and small % 16 == 0
    assert large >= 2 * 4 * (3 * (10_000_000 // 2048 + 1) + 1)


def test_plan_argument_errors(lib):
    plan = lib.gs_densify_plan
    need = lib.gs_densify_plan_scratch_bytes(100)
    assert plan(0, None, None, None, 2, 0, None, None, None, 0, None) == 0  # an empty call
    for children in (0, 9, -1):
        assert plan(100, None, None, None, children, 200, FAKE, FAKE, FAKE, need, None) == -1
        assert b"children" in err(lib)
    assert plan(-1, None, None, None, 2, 200, FAKE, FAKE, FAKE, need, None) == -1
    assert plan(100, None, None, None, 2, -1, FAKE, FAKE, FAKE, need, None) == -1 and b"capacity" in err(lib)
    # n * max(2, children) < 2^31
    assert plan(2 ** 30, None, None, None, 1, 8, FAKE, FAKE, FAKE, 1 << 40, None) == -1 and b"2^31" in err(lib)
    assert plan(2 ** 28, None, None, None, 8, 8, FAKE, FAKE, FAKE, 1 << 40, None) == -1 and b"2^31" in err(lib)
    assert plan(2 ** 31, None, None, None, 2, 8, FAKE, FAKE, FAKE, 1 << 40, None) == -1
    # NULL buffers
    assert plan(100, None, None, None, 2, 200, None, FAKE, FAKE, need, None) == -1 and b"NULL" in err(lib)
    assert plan(100, None, None, None, 2, 200, FAKE, None, FAKE, need, None) == -1 and b"NULL" in err(lib)
    # scratch: missing, short, misaligned
    assert plan(100, None, None, None, 2, 200, FAKE, FAKE, None, need, None) == -4
    assert plan(100, None, None, None, 2, 200, FAKE, FAKE, FAKE, need - 1, None) == -4 and b"scratch" in err(lib)
    assert plan(100, None, None, None, 2, 200, FAKE, FAKE, FAKE + 8, need, None) == -1 and b"aligned" in err(lib)
    with pytest.raises(ValueError):
        _native.check(-1, "gs_densify_plan")


def columns(*specs):
    return (_native.GsMoveColumn * len(specs))(*(_native.GsMoveColumn(*s) for s in specs))


def test_move_argument_errors(lib):
    move = lib.gs_table_move_rows
    one = columns((FAKE, FAKE, 16, 10))
    assert move(0, None, 1, one, None) == 0 and move(10, FAKE, 0, None, None) == 0  # empty calls
    assert move(-1, FAKE, 1, one, None) == -1 and move(2 ** 31, FAKE, 1, one, None) == -1
    for count in (-1, 33):
        assert move(10, FAKE, count, one, None) == -1 and b"columns" in err(lib)
    assert move(10, FAKE, 1, None, None) == -1 and b"NULL" in err(lib)
    for row_bytes in (0, -4, 1, 2, 6, 15):
        assert move(10, FAKE, 1, columns((FAKE, FAKE, row_bytes, 10)), None) == -1 and b"multiple of 4" in err(lib)
    for copy_rows in (-1, 11):
        assert move(10, FAKE, 1, columns((FAKE, FAKE, 16, copy_rows)), None) == -1 and b"copies" in err(lib)
    assert move(10, FAKE, 1, columns((FAKE, None, 16, 10)), None) == -1 and b"NULL" in err(lib)
    assert move(10, FAKE, 1, columns((None, FAKE, 16, 10)), None) == -1 and b"NULL" in err(lib)
    assert move(10, None, 1, one, None) == -1 and b"src_of" in err(lib)
    assert move(10, FAKE, 1, columns((FAKE + 2, FAKE, 16, 10)), None) == -1 and b"aligned" in err(lib)
    # the second column is the bad one
    assert move(10, FAKE, 2, columns((FAKE, FAKE, 16, 10), (FAKE, FAKE, 16, 12)), None) == -1
    assert b"column 1" in err(lib)
    # 32-bit unit counts: 2^30 rows of 64 bytes are 2^32 16-byte units
    assert move(2 ** 30, FAKE, 1, columns((FAKE, FAKE, 64, 0)), None) == -2 and b"2^32" in err(lib)


def test_split_argument_errors(lib):
    split = lib.gs_split3d_children
    assert split(0, 2, None, None, None, None, None, 0.47, None, None, None) == 0  # an empty call
    for children in (0, 9):
        assert split(8, children, FAKE, FAKE, FAKE, FAKE, FAKE, 0.47, FAKE, FAKE, None) == -1
        assert b"children" in err(lib)
    assert split(-2, 2, FAKE, FAKE, FAKE, FAKE, FAKE, 0.47, FAKE, FAKE, None) == -1
    assert split(7, 2, FAKE, FAKE, FAKE, FAKE, FAKE, 0.47, FAKE, FAKE, None) == -1  # not children * parents
    assert split(2 ** 31, 2, FAKE, FAKE, FAKE, FAKE, FAKE, 0.47, FAKE, FAKE, None) == -1
    for hole in range(7):
        args = [FAKE] * 7
        args[hole] = None
        assert split(8, 2, *args[:5], 0.47, *args[5:], None) == -1 and b"NULL" in err(lib)


def test_accumulate_argument_errors(lib):
    acc = lib.gs_densify_accumulate
    assert acc(0, 5, None, None, 0, None, None, None, None, None) == 0  # empty calls
    assert acc(5, 0, None, None, 0, None, None, None, None, None) == 0
    assert acc(-1, 5, FAKE, None, 0, None, None, None, FAKE, None) == -1
    assert acc(5, -1, FAKE, None, 0, None, None, None, FAKE, None) == -1
    assert acc(2 ** 31, 5, FAKE, None, 0, None, None, None, FAKE, None) == -1
    assert acc(5, 2 ** 31, FAKE, None, 0, None, None, None, FAKE, None) == -1
    assert acc(5, 5, None, None, 0, None, None, None, FAKE, None) == -1 and b"NULL" in err(lib)
    assert acc(5, 5, FAKE, None, 0, None, None, None, None, None) == -1 and b"NULL" in err(lib)
    assert acc(5, 5, FAKE, FAKE, 1, None, None, None, FAKE, None) == -1 and b"stride" in err(lib)


# ---- the Python layer: refused before any launch (CPU tensors would raise the device error only after these)
def mask(n, value=False):
    return torch.full((n,), value, dtype=torch.bool)


def test_plan_densify_refuses_bad_masks():
    with pytest.raises(TypeError, match="bool"):
        gs.plan_densify(prune=torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(TypeError, match="bool"):
        gs.plan_densify(split=torch.zeros(8))
    with pytest.raises(TypeError, match="Tensor"):
        gs.plan_densify(clone=[True, False])
    with pytest.raises(ValueError, match="shape"):
        gs.plan_densify(prune=torch.zeros((8, 1), dtype=torch.bool))
    with pytest.raises(ValueError, match="shape"):
        gs.plan_densify(prune=mask(8), split=mask(9))
    with pytest.raises(ValueError, match="no mask"):
        gs.plan_densify()
    for children in (0, 9):
        with pytest.raises(ValueError, match="children"):
            gs.plan_densify(prune=mask(8), children=children)
    with pytest.raises(ValueError, match="max_rows"):
        gs.plan_densify(prune=mask(8), max_rows=-1)
    with pytest.raises(RuntimeError, match="HIP device"):  # well-formed, but on the CPU: no fallback
        gs.plan_densify(prune=mask(8))


def cpu_plan(n=6, kept=4, clones=1, parents=2, children=2):
    rows = kept + clones + children * parents
    return gs.DensifyPlan(torch.zeros(rows, dtype=torch.int32), kept, clones, parents, rows, children, n)


def cpu_params(n=6, drop=()):
    table = dict(position=torch.zeros(n, 3), log_scaling=torch.zeros(n, 3), rotation=torch.ones(n, 4),
                 alpha_logit=torch.zeros(n, 1), feature=torch.zeros(n, 3))
    table = {k: v for k, v in table.items() if k not in drop}
    return ParameterClass(table, {k: dict(lr=0.1) for k in table}, optimizer=torch.optim.Adam)


def test_densify_refuses_bad_arguments():
    plan = cpu_plan()
    assert plan.num_children == 4 and plan.first_child == 5
    with pytest.raises(ValueError, match="state"):
        gs.densify(cpu_params(), plan, state="copy")
    with pytest.raises(ValueError, match="rotation"):
        gs.densify(cpu_params(drop=("rotation",)), plan)
    for bad in (torch.zeros(4, 2), torch.zeros(3, 3), torch.zeros(2, 2, 3)):
        with pytest.raises(ValueError, match="noise"):
            gs.densify(cpu_params(), plan, noise=bad)
    with pytest.raises(TypeError, match="float32"):
        gs.densify(cpu_params(), plan, noise=torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="shrink"):
        gs.densify(cpu_params(), plan, shrink=0.0)
    with pytest.raises(ValueError, match="6 rows"):  # a table of another size than the plan's
        gs.densify(cpu_params(n=7), plan)
    with pytest.raises(RuntimeError, match="HIP device"):
        gs.densify(cpu_params(), plan, noise=torch.zeros(4, 3))
    # a plan without split rows needs no rotation; it gets as far as the device check
    with pytest.raises(RuntimeError, match="HIP device"):
        gs.densify(cpu_params(drop=("rotation",)), cpu_plan(parents=0))


def test_move_rows_and_split_refuse_bad_arguments():
    plan = cpu_plan()
    with pytest.raises(ValueError, match="copy_rows"):
        gs.move_rows(dict(a=torch.zeros(6)), plan, copy_rows=plan.rows + 1)
    with pytest.raises(ValueError, match="6 rows"):
        gs.move_rows(dict(a=torch.zeros(5)), plan)
    with pytest.raises(RuntimeError, match="HIP device"):
        gs.move_rows(dict(a=torch.zeros(6)), plan)
    g = gs.Gaussians3D(position=torch.zeros(6, 3), log_scaling=torch.zeros(6, 3), rotation=torch.ones(6, 4),
                       alpha_logit=torch.zeros(6, 1), feature=torch.zeros(6, 3))
    for bad in (torch.zeros(6, 3), torch.zeros(5, 2, 3), torch.zeros(6, 2, 2), torch.zeros(6, 9, 3)):
        with pytest.raises(ValueError):
            gs.split_gaussians3d(g, bad)
    with pytest.raises(RuntimeError, match="HIP device"):
        gs.split_gaussians3d(g, torch.zeros(6, 2, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        gs.DensifyStats(6, "cpu")
