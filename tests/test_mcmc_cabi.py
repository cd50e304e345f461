"""The MCMC strategy without a GPU: the entry points are exported and bound, every argument error is reported by the host
before any launch, the Python layer refuses bad arguments before it touches the device, and the numpy reference gives
hand-computed answers."""
import ctypes
import math

import numpy as np
import pytest
import torch

import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import _native, mcmc
from taichi_gaussian_rasterizer_amd.optim import ParameterClass

from mcmc_reference import (quantise, reference_perturb, reference_sample, reference_values, scaled_draw)

FAKE = 0x10000  # a non-NULL, 16-byte aligned address: validation fails before anything could read it
ENTRY_POINTS = {"gs_sample_rows_scratch_bytes": 1, "gs_sample_rows": 11, "gs_mcmc_relocation_values": 8,
                "gs_mcmc_apply": 8, "gs_table_relocate_rows": 7, "gs_mcmc_perturb": 10}
PUBLIC = ("Relocation", "grow", "perturb", "relocate", "relocation_values", "sample_rows")


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.lib()


def err(lib):
    return lib.gs_last_error()


def test_exports_and_bindings(lib):
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name, args in ENTRY_POINTS.items():
        assert hasattr(handle, name), name
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == args, name
    for name in PUBLIC:
        assert name in gs.__all__ and getattr(gs, name) is getattr(mcmc, name), name
        assert name in mcmc.__all__


def test_constants_and_struct_layout():
    assert _native.GS_MCMC_N_MAX == 51
    assert (_native.GS_RELOCATE_COPY, _native.GS_RELOCATE_ZERO, _native.GS_RELOCATE_ZERO_SOURCES) == (0, 1, 2)
    column = _native.GsRelocateColumn
    assert ctypes.sizeof(column) == 16
    assert (column.data.offset, column.row_bytes.offset, column.mode.offset) == (0, 8, 12)
    header = open(_native.os.path.join(_native._HERE, "..", "include", "gsplat_hip.h")).read()
    for text in ("#define GS_MCMC_N_MAX 51", "#define GS_RELOCATE_COPY 0", "#define GS_RELOCATE_ZERO 1",
                 "#define GS_RELOCATE_ZERO_SOURCES 2"):
        assert text in header, text


def test_scratch_size(lib):
    size = lib.gs_sample_rows_scratch_bytes
    assert size(0) == 0 and size(-5) == 0
    sizes = [size(n) for n in (1, 2, 2047, 2048, 2049, 65536, 1_000_000, 2 ** 21 + 1, 2 ** 31 - 1)]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert sizes == sorted(sizes)
    assert size(1_000_000) >= 1_000_000 * 8  # at least the uint64 prefix


def test_sample_rows_argument_errors(lib):
    sample = lib.gs_sample_rows
    need = lib.gs_sample_rows_scratch_bytes(100)
    assert sample(0, None, None, 0, None, None, None, None, None, 0, None) == 0  # an empty call touches no pointer
    assert sample(-1, FAKE, None, 5, FAKE, None, FAKE, None, FAKE, need, None) == -1 and b"rows" in err(lib)
    assert sample(2 ** 31, FAKE, None, 5, FAKE, None, FAKE, None, FAKE, 1 << 50, None) == -1 and b"2^31" in err(lib)
    assert sample(100, FAKE, None, -1, FAKE, None, FAKE, None, FAKE, need, None) == -1 and b"draws" in err(lib)
    assert sample(100, FAKE, None, 2 ** 31, FAKE, None, FAKE, None, FAKE, need, None) == -1 and b"draws" in err(lib)
    assert sample(100, FAKE, None, 5, FAKE, FAKE, FAKE, None, FAKE, need, None) == -1 and b"select" in err(lib)
    assert sample(0, FAKE, None, 5, FAKE, None, FAKE, None, FAKE, need, None) == -1 and b"empty" in err(lib)
    assert sample(100, None, None, 5, FAKE, None, FAKE, None, FAKE, need, None) == -1 and b"weights" in err(lib)
    assert sample(100, FAKE, None, 5, None, None, FAKE, None, FAKE, need, None) == -1 and b"random" in err(lib)
    assert sample(100, FAKE, None, 5, FAKE, None, None, None, FAKE, need, None) == -1 and b"out" in err(lib)
    assert sample(100, FAKE, None, 5, FAKE, None, FAKE, None, None, need, None) == -1 and b"scratch" in err(lib)
    assert sample(100, FAKE, None, 5, FAKE, None, FAKE, None, FAKE, need - 1, None) == -4 and b"scratch" in err(lib)
    assert sample(100, FAKE, None, 5, FAKE, None, FAKE, None, FAKE + 8, need, None) == -1 and b"aligned" in err(lib)
    assert sample(100, FAKE + 2, None, 5, FAKE, None, FAKE, None, FAKE, need, None) == -1 and b"aligned" in err(lib)
    assert sample(100, FAKE, None, 5, FAKE, None, FAKE, FAKE + 1, FAKE, need, None) == -1 and b"aligned" in err(lib)
    with pytest.raises(RuntimeError):
        _native.check(-4, "gs_sample_rows")


def test_relocation_values_and_apply_argument_errors(lib):
    values, apply = lib.gs_mcmc_relocation_values, lib.gs_mcmc_apply
    assert values(0, None, None, None, 0.005, None, None, None) == 0
    assert values(-1, FAKE, FAKE, FAKE, 0.005, FAKE, FAKE, None) == -1 and b"rows" in err(lib)
    assert values(2 ** 31, FAKE, FAKE, FAKE, 0.005, FAKE, FAKE, None) == -1 and b"2^31" in err(lib)
    for bad in (0.0, 1.0, -0.5, math.nan):
        assert values(10, FAKE, FAKE, FAKE, bad, FAKE, FAKE, None) == -1 and b"min_opacity" in err(lib)
    for k in range(5):
        args = [FAKE] * 5
        args[k] = None
        assert values(10, args[0], args[1], args[2], 0.005, args[3], args[4], None) == -1 and b"NULL" in err(lib)
    assert apply(0, None, None, None, None, None, None, None) == 0
    assert apply(-1, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None) == -1 and b"rows" in err(lib)
    assert apply(2 ** 31, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None) == -1 and b"2^31" in err(lib)
    for k in range(6):
        args = [FAKE] * 6
        args[k] = None
        assert apply(10, *args, None) == -1 and b"NULL" in err(lib)


def test_relocate_rows_argument_errors(lib):
    move = lib.gs_table_relocate_rows
    column = _native.GsRelocateColumn

    def call(n, src_of, select, copies, *columns):
        arr = (column * max(len(columns), 1))(*columns)
        return move(n, src_of, select, copies, len(columns), arr, None)

    good = column(FAKE, 12, _native.GS_RELOCATE_COPY)
    assert move(0, None, None, None, 1, None, None) == 0 and move(10, None, None, None, 0, None, None) == 0
    assert call(-1, FAKE, FAKE, FAKE, good) == -1 and b"rows" in err(lib)
    assert call(2 ** 31, FAKE, FAKE, FAKE, good) == -1 and b"rows" in err(lib)
    assert move(10, FAKE, FAKE, FAKE, 33, None, None) == -1 and b"columns" in err(lib)
    assert move(10, FAKE, FAKE, FAKE, -1, None, None) == -1 and b"columns" in err(lib)
    assert move(10, FAKE, FAKE, FAKE, 1, None, None) == -1 and b"NULL" in err(lib)
    for row_bytes in (0, 6, -4, 1):
        assert call(10, FAKE, FAKE, FAKE, column(FAKE, row_bytes, 0)) == -1 and b"multiple of 4" in err(lib)
    for mode in (-1, 3):
        assert call(10, FAKE, FAKE, FAKE, column(FAKE, 12, mode)) == -1 and b"mode" in err(lib)
    assert call(10, FAKE, FAKE, FAKE, column(None, 12, 0)) == -1 and b"NULL" in err(lib)
    assert call(10, FAKE, FAKE, FAKE, good, column(FAKE + 2, 12, 1)) == -1 and b"column 1" in err(lib)
    assert call(10, None, FAKE, FAKE, good) == -1 and b"src_of" in err(lib)
    assert call(10, FAKE, None, FAKE, good) == -1 and b"select" in err(lib)
    assert call(10, None, FAKE, FAKE, column(FAKE, 12, _native.GS_RELOCATE_ZERO)) == -1 and b"src_of" in err(lib)
    assert call(10, FAKE, None, FAKE, column(FAKE, 12, _native.GS_RELOCATE_ZERO)) == -1 and b"select" in err(lib)
    assert call(10, FAKE, FAKE, None, column(FAKE, 12, _native.GS_RELOCATE_ZERO)) == -1 and b"copies" in err(lib)
    assert call(10, None, None, None, column(FAKE, 12, _native.GS_RELOCATE_ZERO_SOURCES)) == -1 and b"copies" in err(lib)
    # 8-byte rows at an address that is no multiple of 16 go as 4-byte units: 2^32 - 2 of them, past the limit
    assert call(2 ** 31 - 1, FAKE, FAKE, FAKE, column(FAKE + 4, 8, 0)) == -2 and b"units" in err(lib)
    with pytest.raises(NotImplementedError):
        _native.check(-2, "gs_table_relocate_rows")


def test_perturb_argument_errors(lib):
    perturb = lib.gs_mcmc_perturb
    assert perturb(0, None, None, None, None, None, 1.0, 100.0, 0.995, None) == 0
    assert perturb(-1, FAKE, FAKE, FAKE, FAKE, FAKE, 1.0, 100.0, 0.995, None) == -1 and b"rows" in err(lib)
    assert perturb(2 ** 31, FAKE, FAKE, FAKE, FAKE, FAKE, 1.0, 100.0, 0.995, None) == -1 and b"2^31" in err(lib)
    for k in range(5):
        args = [FAKE] * 5
        args[k] = None
        assert perturb(10, *args, 1.0, 100.0, 0.995, None) == -1 and b"NULL" in err(lib)
    assert perturb(10, FAKE, FAKE, FAKE + 4, FAKE, FAKE, 1.0, 100.0, 0.995, None) == -1 and b"aligned" in err(lib)


# ---- the Python layer
def cpu_params(n=8, without=()):
    columns = dict(position=torch.zeros(n, 3), log_scaling=torch.zeros(n, 3), rotation=torch.ones(n, 4),
                   alpha_logit=torch.zeros(n, 1), feature=torch.zeros(n, 3))
    columns = {name: t for name, t in columns.items() if name not in without}
    return ParameterClass(columns, {name: dict(lr=1e-3) for name in columns}, optimizer=torch.optim.Adam)


def test_sample_rows_refuses_bad_arguments():
    good = torch.rand(8)
    with pytest.raises(TypeError, match="Tensor"):
        gs.sample_rows([0.5, 0.5])
    for dtype in (torch.float64, torch.float16, torch.int32):
        with pytest.raises(TypeError, match="float32"):
            gs.sample_rows(torch.zeros(8, dtype=dtype))
    for shape in ((8, 1), (2, 4), ()):
        with pytest.raises(ValueError, match="shape"):
            gs.sample_rows(torch.zeros(shape))
    with pytest.raises(ValueError, match="draws"):
        gs.sample_rows(good, -1)
    with pytest.raises(TypeError, match="exclude"):
        gs.sample_rows(good, exclude=torch.zeros(8))
    with pytest.raises(ValueError, match="exclude"):
        gs.sample_rows(good, exclude=torch.zeros(7, dtype=torch.bool))
    with pytest.raises(ValueError, match="select"):
        gs.sample_rows(good, 5, select=torch.zeros(5, dtype=torch.bool))  # m != n
    with pytest.raises(TypeError, match="random"):
        gs.sample_rows(good, random=torch.rand(8))
    with pytest.raises(ValueError, match="random"):
        gs.sample_rows(good, 5, random=torch.zeros(8, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="HIP device"):  # well-formed, but on the CPU: no fallback
        gs.sample_rows(good, 5, random=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="HIP device"):
        gs.sample_rows(torch.zeros(0), 0)


def test_relocation_values_refuses_bad_arguments():
    o, ls, c = torch.rand(8), torch.zeros(8, 3), torch.ones(8, dtype=torch.int32)
    with pytest.raises(TypeError, match="copies"):
        gs.relocation_values(o, ls, c.long())
    with pytest.raises(TypeError, match="float32"):
        gs.relocation_values(o.double(), ls, c)
    with pytest.raises(TypeError, match="float32"):
        gs.relocation_values(o, ls.double(), c)
    with pytest.raises(ValueError, match="opacity"):
        gs.relocation_values(torch.rand(7), ls, c)
    with pytest.raises(ValueError, match="log_scaling"):
        gs.relocation_values(o, torch.zeros(8, 2), c)
    for bad in (0.0, 1.0, math.nan):
        with pytest.raises(ValueError, match="min_opacity"):
            gs.relocation_values(o, ls, c, min_opacity=bad)
    with pytest.raises(RuntimeError, match="HIP device"):
        gs.relocation_values(o, ls, c)


def test_relocate_and_grow_refuse_bad_arguments():
    params, dead = cpu_params(), torch.zeros(8, dtype=torch.bool)
    with pytest.raises(ValueError, match="state"):
        gs.relocate(params, dead, state="parent")
    with pytest.raises(TypeError, match="ParameterClass"):
        gs.relocate(dict(params.items()), dead)
    for missing in ("alpha_logit", "log_scaling"):
        with pytest.raises(ValueError, match=missing):
            gs.relocate(cpu_params(without=(missing,)), dead)
        with pytest.raises(ValueError, match=missing):
            gs.grow(cpu_params(without=(missing,)), 2)
    with pytest.raises(TypeError, match="bool"):
        gs.relocate(params, dead.float())
    with pytest.raises(ValueError, match="dead"):
        gs.relocate(params, dead[:7])
    with pytest.raises(ValueError, match="random"):
        gs.relocate(params, dead, random=torch.zeros(7, dtype=torch.int64))
    with pytest.raises(ValueError, match="min_opacity"):
        gs.relocate(params, dead, min_opacity=2.0)
    double = ParameterClass({name: t.detach().double() for name, t in params.items()},
                            {name: dict(lr=1e-3) for name in params.keys()}, optimizer=torch.optim.Adam)
    with pytest.raises(TypeError, match="float32"):
        gs.relocate(double, dead)
    with pytest.raises(TypeError, match="float32"):
        gs.grow(double, 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        gs.relocate(params, dead)
    with pytest.raises(RuntimeError, match="HIP device"):
        gs.grow(params, 2)
    with pytest.raises(ValueError, match="random"):
        gs.grow(params, 2, random=torch.zeros(3, dtype=torch.int64))
    # nothing to add: the same object, whatever the device
    assert gs.grow(params, 0) is params and gs.grow(params, -3) is params and gs.grow(params, 5, max_rows=8) is params


def test_perturb_refuses_bad_arguments():
    params = cpu_params()
    table = {name: t.detach() for name, t in params.items()}
    with pytest.raises(TypeError, match="mapping"):
        gs.perturb(table["position"], 1e-4)
    with pytest.raises(ValueError, match="rotation"):
        gs.perturb({k: v for k, v in table.items() if k != "rotation"}, 1e-4)
    with pytest.raises(TypeError, match="float32"):
        gs.perturb({**table, "position": table["position"].double()}, 1e-4)
    with pytest.raises(ValueError, match="rotation"):
        gs.perturb({**table, "rotation": torch.ones(8, 3)}, 1e-4)
    with pytest.raises(ValueError, match="noise"):
        gs.perturb(table, 1e-4, noise=torch.zeros(8, 2))
    with pytest.raises(TypeError, match="noise"):
        gs.perturb(table, 1e-4, noise=torch.zeros(8, 3, dtype=torch.float64))
    for target in (params, table, gs.Gaussians3D(**table)):
        with pytest.raises(RuntimeError, match="HIP device"):
            gs.perturb(target, 1e-4)


# ---- the reference against hand-computed cases
def test_reference_quantise_and_draw():
    below = np.nextafter(np.float32(2.0 ** -24), np.float32(0))
    w = np.array([0, 1, 2.5, -1, np.nan, 1e-42, 2.0 ** -24, below, 0.5], dtype=np.float32)
    assert quantise(w).tolist() == [0, 2 ** 24, 2 ** 24, 0, 0, 0, 1, 0, 2 ** 23]
    assert quantise(w, exclude=[0, 1, 0, 0, 0, 0, 0, 0, 0]).tolist() == [0, 0, 2 ** 24, 0, 0, 0, 1, 0, 2 ** 23]
    for total in (1, 2 ** 24, 3 * 2 ** 24 + 1, 2 ** 55 - 1):
        for r in (0, 1, 2 ** 31, 2 ** 32 - 1):
            assert int(scaled_draw([r], total)[0]) == (r * total) >> 32 < total
    # total = 2^24 + 2^24 + 1 + 2^23: r = 0 -> the first row with q > 0; r = 2^32 - 1 -> the last one
    rows, copies = reference_sample(w, [0, 2 ** 32 - 1, 2 ** 31])
    assert rows.tolist() == [1, 8, 2] and copies.tolist() == [0, 1, 1, 0, 0, 0, 0, 0, 1]
    rows, copies = reference_sample(w, [7] * 9, select=[1, 0, 0, 0, 0, 0, 0, 0, 1])
    assert rows.tolist() == [1, 1, 2, 3, 4, 5, 6, 7, 1] and copies[1] == 2
    rows, copies = reference_sample(np.zeros(4, np.float32), [5, 6, 7, 8])
    assert rows.tolist() == [0, 1, 2, 3] and not copies.any()


def test_reference_values_closed_forms():
    # n = 2: denom = 2 x - x^2 / sqrt(2) with x = 1 - sqrt(1 - o)
    o = np.float32(0.3)
    alpha, ls = reference_values([o], np.zeros((1, 3), np.float32), [1])
    x = 1 - math.sqrt(1 - float(o))
    assert alpha[0] == pytest.approx(math.log(x / (1 - x)), rel=1e-14)
    assert ls[0, 0] == pytest.approx(math.log(float(o) / (2 * x - x * x / math.sqrt(2))), rel=1e-13)
    # saturation at 51 and the clamp at both ends
    a500, s500 = reference_values([o], np.zeros((1, 3), np.float32), [500])
    a50, s50 = reference_values([o], np.zeros((1, 3), np.float32), [50])
    assert a500[0] == a50[0] and (s500 == s50).all()
    alpha, ls = reference_values([np.float32(1.0)], np.zeros((1, 3), np.float32), [1])
    assert alpha[0] == pytest.approx(math.log((1 - 2.0 ** -23) * 2.0 ** 23)) and np.isfinite(ls).all()
    alpha, _ = reference_values([np.float32(1e-6)], np.zeros((1, 3), np.float32), [9])
    assert alpha[0] == pytest.approx(math.log(float(np.float32(0.005)) / (1 - float(np.float32(0.005)))))
    alpha, ls = reference_values([o, o], np.ones((2, 3), np.float32), [0, 1])
    assert np.isnan(alpha[0]) and (ls[0] == 1).all()


def test_reference_perturb_identity_rotation():
    ls = np.log(np.array([[1.0, 2.0, 3.0]], dtype=np.float32))
    noise = np.array([[1.0, 1.0, 1.0]], dtype=np.float32)
    a = np.array([[math.log(0.005 / 0.995)]], dtype=np.float32)  # o = 0.005: the exponent is 0, the gate 1/2
    d, g, exponent = reference_perturb(ls, [[0, 0, 0, 2.0]], a, noise, scale=4.0)
    assert g[0] == pytest.approx(0.5, abs=1e-5) and abs(exponent[0]) < 1e-5
    assert d[0] == pytest.approx([2.0, 8.0, 18.0], rel=1e-4)
    d, g, _ = reference_perturb(ls, [[0, 0, 0, 2.0]], [[5.0]], noise, scale=4.0)
    assert g[0] < 1e-42 and np.abs(d).max() < 1e-39  # o = 0.993: the float64 gate is exp(-98.8), a float32 one 0
