"""Nearest neighbours without a GPU: the entry points are exported and bound, every argument error is reported by the
host before any launch, the Python layer refuses bad arguments before it touches the device, and the brute-force oracle
gives the hand-computed answers."""
import ctypes
import math

import numpy as np
import pytest
import torch

import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import _native, neighbours

from knn_reference import reference_knn

FAKE = 0x10000  # a non-NULL, 16-byte aligned address: validation fails before anything could read it
INF = math.inf


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.lib()


def err(lib):
    return lib.gs_last_error()


def test_exports_and_bindings(lib):
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in ("gs_knn3d_scratch_bytes", "gs_knn3d"):
        assert hasattr(handle, name), name
        assert name in _native.SIGNATURES, name
    assert len(_native.SIGNATURES["gs_knn3d"][1]) == 8 and len(_native.SIGNATURES["gs_knn3d_scratch_bytes"][1]) == 1
    assert _native.GS_KNN_MAX == 16
    for name in ("knn", "gaussians_from_points"):
        assert name in gs.__all__ and getattr(gs, name) is getattr(neighbours, name), name


def test_scratch_size(lib):
    size = lib.gs_knn3d_scratch_bytes
    assert size(0) == 0 and size(-5) == 0
    sizes = [size(n) for n in (1, 2, 255, 256, 257, 1000, 4097, 65536, 1_000_000, 10_000_000, 2 ** 31 - 1)]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert sizes == sorted(sizes)
    assert size(1_000_000) >= 1_000_000 * 16  # at least the packed records


def test_argument_errors(lib):
    knn = lib.gs_knn3d
    need = lib.gs_knn3d_scratch_bytes(100)
    assert knn(0, None, 3, None, None, None, 0, None) == 0  # an empty call touches no pointer
    assert knn(-1, FAKE, 3, FAKE, FAKE, FAKE, need, None) == -1 and b"points" in err(lib)
    assert knn(2 ** 31, FAKE, 3, FAKE, FAKE, FAKE, 1 << 50, None) == -1 and b"2^31" in err(lib)
    for k in (0, 17, -1):
        assert knn(100, FAKE, k, FAKE, FAKE, FAKE, need, None) == -1 and b"k " in err(lib) and b"16" in err(lib)
        assert knn(0, None, k, None, None, None, 0, None) == -1  # also refused for an empty cloud
    assert knn(100, None, 3, FAKE, FAKE, FAKE, need, None) == -1 and b"NULL" in err(lib) and b"points" in err(lib)
    assert knn(100, FAKE, 3, None, FAKE, FAKE, need, None) == -1 and b"NULL" in err(lib) and b"dist2" in err(lib)
    assert knn(100, FAKE, 3, FAKE, FAKE, None, need, None) == -1 and b"NULL" in err(lib) and b"scratch" in err(lib)
    assert knn(100, FAKE, 3, FAKE, FAKE, FAKE, need - 1, None) == -4 and b"scratch" in err(lib)
    assert knn(100, FAKE, 3, FAKE, None, FAKE, 0, None) == -4  # a NULL index is allowed; the scratch is still short
    assert knn(100, FAKE, 3, FAKE, FAKE, FAKE + 8, need, None) == -1 and b"aligned" in err(lib)
    with pytest.raises(RuntimeError):
        _native.check(-4, "gs_knn3d")


def test_knn_refuses_bad_arguments():
    good = torch.zeros(8, 3)
    with pytest.raises(TypeError, match="Tensor"):
        gs.knn([[0.0, 0.0, 0.0]])
    with pytest.raises(TypeError, match="Tensor"):
        gs.knn(np.zeros((8, 3), dtype=np.float32))
    for dtype in (torch.float64, torch.float16, torch.int32):
        with pytest.raises(TypeError, match="float32"):
            gs.knn(torch.zeros(8, 3, dtype=dtype))
    for shape in ((8,), (8, 2), (8, 4), (2, 8, 3), (3, 8)):
        with pytest.raises(ValueError, match="shape"):
            gs.knn(torch.zeros(shape))
    for k in (0, 17, -3):
        with pytest.raises(ValueError, match="k "):
            gs.knn(good, k=k)
    with pytest.raises(RuntimeError, match="HIP device"):  # well-formed, but on the CPU: no fallback
        gs.knn(good, k=3)
    with pytest.raises(RuntimeError, match="HIP device"):
        gs.knn(torch.zeros(0, 3), k=1, return_index=False)


def test_gaussians_from_points_refuses_bad_arguments():
    points, colors = torch.zeros(8, 3), torch.full((8, 3), 0.5)
    make = gs.gaussians_from_points
    with pytest.raises(TypeError, match="float32"):
        make(points.double())
    with pytest.raises(ValueError, match="shape"):
        make(torch.zeros(8, 2))
    for k in (0, 17):
        with pytest.raises(ValueError, match="k "):
            make(points, k=k)
    for alpha in (0.0, 1.0, -0.1, 1.5, math.nan):
        with pytest.raises(ValueError, match="initial_alpha"):
            make(points, initial_alpha=alpha)
    for factor in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="scale_factor"):
            make(points, scale_factor=factor)
    with pytest.raises(ValueError, match="min_scale"):
        make(points, min_scale=1.0, max_scale=0.5)
    with pytest.raises(ValueError, match="sh_degree"):
        make(points, colors, sh_degree=4)
    with pytest.raises(TypeError, match="colors"):
        make(points, colors.double())
    for bad in (torch.zeros(7, 3), torch.zeros(8), torch.zeros(8, 3, 1)):
        with pytest.raises(ValueError, match="colors"):
            make(points, bad)
    with pytest.raises(ValueError, match="spherical harmonics"):
        make(points, torch.zeros(8, 4), sh_degree=1)
    with pytest.raises(ValueError, match="colors on"):
        make(points, colors.to("meta"))
    for kwargs in (dict(), dict(colors=colors), dict(colors=colors, sh_degree=2), dict(colors=torch.zeros(8, 5))):
        with pytest.raises(RuntimeError, match="HIP device"):
            make(points, **kwargs)


def test_neighbour_scale_formula():
    d2 = torch.tensor([[1.0, 4.0, 7.0], [4.0, INF, INF], [INF, INF, INF], [0.0, 0.0, 0.0], [1e10, 1e10, 1e10]])
    scale = neighbours.neighbour_scale(d2, scale_factor=0.5, min_scale=1e-3, max_scale=100.0)
    assert scale.tolist() == [1.0, 1.0, pytest.approx(1e-3), pytest.approx(1e-3), 100.0]


# ---- the oracle against hand-computed cases
def test_oracle_collinear():
    p = np.zeros((4, 3), dtype=np.float32)
    p[:, 0] = (0, 1, 3, 7)
    d2, j = reference_knn(p, 2)
    assert d2.dtype == np.float32 and j.dtype == np.int64
    assert d2.tolist() == [[1, 9], [1, 4], [4, 9], [16, 36]]
    assert j.tolist() == [[1, 2], [0, 2], [1, 0], [2, 1]]


def test_oracle_identical_points():
    d2, j = reference_knn(np.full((3, 3), 2.5, dtype=np.float32), 3)
    assert d2.tolist() == [[0, 0, INF]] * 3  # two duplicates at distance 0, then padding
    assert j.tolist() == [[1, 2, -1], [0, 2, -1], [0, 1, -1]]  # ties by index, the point itself removed by index


def test_oracle_non_finite_and_operation_order():
    p = np.array([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0], [0, np.inf, 0]], dtype=np.float32)
    d2, j = reference_knn(p, 2)
    assert j.tolist() == [[2, -1], [-1, -1], [0, -1], [-1, -1]]
    assert d2[0, 0] == 1 and np.isinf(d2[1]).all() and np.isinf(d2[3]).all()
    # (dx^2 + dy^2) + dz^2 in float32, in this order: differs from the other association for these values
    a = np.array([[0, 0, 0], [1, 2.0 ** -12, 2.0 ** -12]], dtype=np.float32)
    one, tiny = np.float32(1), np.float32(2.0 ** -24)
    assert reference_knn(a, 1)[0][0, 0] == (one + tiny) + tiny == one
    assert one + (tiny + tiny) != one
