"""knn / gs_knn3d on the device against the brute-force float32 oracle (tests/knn_reference.py).  The kernel is exact:
the squared distances are compared as bit patterns and the indices with ==, for every case."""
import math

import numpy as np
import pytest
import torch

import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import RasterConfig, neighbours, scenes

from knn_reference import reference_knn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K_MAX = 16
KS = (1, 3, 4, 5, 16)  # both register capacities (4 and 16) and a k just above the smaller one
SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1000, 4097)


def cube(n, seed=0, offset=0.0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 3, generator=gen) + offset).float()


_ORACLE = {}


def oracle(name, points):
    """the oracle's 16 neighbours of a named point set, computed once; a row's first k entries are its k-neighbour row"""
    if name not in _ORACLE:
        _ORACLE[name] = reference_knn(points.numpy(), K_MAX)
    return _ORACLE[name]


def check(name, points, ks=KS, **kwargs):
    ref_d2, ref_j = oracle(name, points)
    on_device = points.to(DEV)
    for k in ks:
        d2, j = gs.knn(on_device, k, **kwargs)
        assert d2.shape == (points.shape[0], k) and d2.dtype == torch.float32 and not d2.requires_grad
        assert j.shape == (points.shape[0], k) and j.dtype == torch.int64
        got_d2, got_j = d2.cpu().numpy(), j.cpu().numpy()
        bad = np.flatnonzero((got_d2.view(np.int32) != ref_d2[:, :k].view(np.int32)).any(axis=1) |
                             (got_j != ref_j[:, :k]).any(axis=1))
        assert bad.size == 0, (f"{name} k={k}: {bad.size} rows differ, first {bad[0]}: got {got_d2[bad[0]]} "
                               f"{got_j[bad[0]]}, expected {ref_d2[bad[0], :k]} {ref_j[bad[0], :k]}")


@pytest.mark.parametrize("n", SIZES)
def test_uniform_cube(n):
    check(f"cube{n}", cube(n, seed=n))


def test_small_cluster_far_from_the_rest():
    gen = torch.Generator().manual_seed(1)
    near = 0.01 * torch.randn(3, 3, generator=gen)
    far = torch.randn(1000, 3, generator=gen) + torch.tensor([100.0, 0.0, 0.0])
    check("clusters", torch.cat([near, far]), ks=(4,))  # the third and fourth neighbours of the 3 lie in the far runs


def test_identical_points():
    points = torch.full((1000, 3), 0.375)
    check("identical", points, ks=(3, 16))
    d2, j = gs.knn(points.to(DEV), 3)
    assert (d2 == 0).all()
    assert j[0].tolist() == [1, 2, 3] and j[1].tolist() == [0, 2, 3] and j[999].tolist() == [0, 1, 2]


def test_line_and_plane():
    line = torch.zeros(1000, 3)
    line[:, 0] = cube(1000, seed=2)[:, 0] * 10 - 5
    line[:, 1:] = torch.tensor([2.0, -3.0])
    check("line", line, ks=(3, 5))
    plane = cube(1000, seed=3)
    plane[:, 2] = 0.0
    check("plane", plane, ks=(3, 5))


def test_lattice_cut_inside_a_tie_group():
    axis = torch.arange(16, dtype=torch.float32) * 0.25
    points = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), dim=-1).reshape(-1, 3)
    check("lattice", points, ks=(8,))  # an inner point: 6 neighbours at 1/16, then 12 at 1/8: the index rule decides
    d2 = oracle("lattice", points)[0]
    inner = (8 * 16 + 8) * 16 + 8
    assert d2[inner, :6].tolist() == [0.0625] * 6 and d2[inner, 6:8].tolist() == [0.125] * 2


def test_large_offset():
    check("offset", cube(1000, seed=4, offset=1e6), ks=(3, 16))


def test_non_finite_points():
    points = cube(257, seed=5)
    points[0, 1], points[100, 0], points[256, 2] = math.nan, math.inf, -math.inf
    check("nonfinite", points, ks=(3, 16))
    d2, j = gs.knn(points.to(DEV), 16)
    for row in (0, 100, 256):
        assert torch.isinf(d2[row]).all() and (d2[row] > 0).all() and (j[row] == -1).all()
        assert not (j == row).any()


def test_strided_view_no_index_and_streams():
    wide = torch.zeros(1000, 4)
    wide[:, :3] = cube(1000, seed=6)
    view = wide.to(DEV)[:, :3]
    assert not view.is_contiguous()
    check("strided", wide[:, :3].contiguous(), ks=(3,))
    ref_d2 = torch.from_numpy(oracle("strided", None)[0][:, :3]).to(DEV)
    d2, j = gs.knn(view, 3)
    assert torch.equal(d2, ref_d2)
    d2, none = gs.knn(view, 3, return_index=False)
    assert none is None and torch.equal(d2, ref_d2)
    d2, none = gs.knn(view.clone().requires_grad_(True), 5, return_index=False)
    assert not d2.requires_grad
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        d2, j = gs.knn(view, 3)
        total = d2.sum(dim=1) + j.sum(dim=1)  # a dependent torch op on the same stream
    stream.synchronize()
    assert torch.equal(total, ref_d2.sum(dim=1) + torch.from_numpy(oracle("strided", None)[1][:, :3]).to(DEV).sum(dim=1))
    torch.cuda.current_stream(DEV).wait_stream(stream)


@pytest.mark.parametrize("sh_degree", [None, 2])
def test_gaussians_from_points(sh_degree):
    n = 1000
    points = cube(n, seed=7) * 2 - 1 + torch.tensor([0.0, 0.0, 4.0])  # a cube in front of the benchmark camera
    colors = cube(n, seed=8)
    g = gs.gaussians_from_points(points.to(DEV), colors.to(DEV), sh_degree=sh_degree, k=3, initial_alpha=0.3,
                                 scale_factor=0.7, min_scale=1e-4, max_scale=0.2)
    assert tuple(g.batch_size) == (n,)
    for name, shape in (("position", (n, 3)), ("log_scaling", (n, 3)), ("rotation", (n, 4)), ("alpha_logit", (n, 1)),
                        ("feature", (n, 3) if sh_degree is None else (n, 3, 9))):
        t = getattr(g, name)
        assert tuple(t.shape) == shape and t.dtype == torch.float32 and t.device.type == "cuda", name
    assert torch.equal(g.position.cpu(), points)
    # the same formula, on the same device, from the oracle's distances
    ref_d2 = torch.from_numpy(oracle("gfp", points)[0][:, :3]).to(DEV)
    expected = neighbours.neighbour_scale(ref_d2, 0.7, 1e-4, 0.2)
    assert torch.equal(torch.exp(g.log_scaling), torch.exp(torch.log(expected)).unsqueeze(1).repeat(1, 3))
    top = float(np.float32(0.2))  # the clamp's bounds are float32 values
    assert float(expected.min()) >= 1e-4 and float(expected.max()) == top and (expected < top).any()
    assert torch.equal(g.rotation.cpu(), torch.tensor([0.0, 0.0, 0.0, 1.0]).repeat(n, 1))
    assert torch.allclose(torch.sigmoid(g.alpha_logit), torch.full_like(g.alpha_logit, 0.3), atol=1e-6)
    if sh_degree is None:
        assert torch.equal(g.feature.cpu(), colors)
    else:
        # two float32 roundings (the difference, the quotient or the product with the reciprocal)
        assert torch.allclose(g.feature[:, :, 0].cpu(), (colors - 0.5) / 0.2820948, rtol=1e-6, atol=1e-7)
        assert (g.feature[:, :, 1:] == 0).all()
    camera = scenes.benchmark_camera((128, 96)).to(device=DEV)
    rendering = gs.render_gaussians(g, camera, RasterConfig(), use_sh=sh_degree is not None)
    assert rendering.points_in_view.shape[0] > 0
    assert tuple(rendering.image.shape) == (96, 128, 3) and torch.isfinite(rendering.image).all()
    assert float(rendering.image.abs().max()) > 0
    grey = gs.gaussians_from_points(points.to(DEV), sh_degree=sh_degree)
    assert (grey.feature[:, :3] == 0.5).all() if sh_degree is None else (grey.feature == 0).all()


def test_empty_cloud():
    d2, j = gs.knn(torch.zeros(0, 3, device=DEV), 3)
    assert d2.shape == (0, 3) and j.shape == (0, 3) and j.dtype == torch.int64
    g = gs.gaussians_from_points(torch.zeros(0, 3, device=DEV))
    assert tuple(g.position.shape) == (0, 3) and tuple(g.feature.shape) == (0, 3)


def test_single_point_takes_min_scale():
    g = gs.gaussians_from_points(torch.zeros(1, 3, device=DEV), min_scale=0.25)
    assert torch.equal(torch.exp(g.log_scaling), torch.exp(torch.log(torch.full((1, 3), 0.25, device=DEV))))
