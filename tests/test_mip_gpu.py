"""Mip-Splatting's 3D smoothing filter on the device: the sampling rate bit for bit against its float32 restatement, the
smoothing and its gradients against float64 with the float32 numpy evaluation of the same formulas as the yardstick, the
identity and the row-compact backward bit for bit, and the sparse gradients of a frame carried through `smooth3d` into
the optimizers."""
import math

import numpy as np
import pytest
import torch

import mip_reference as ref
import parity_util as pu
import taichi_gaussian_rasterizer_amd as gs
from dense_renderer import render_dense
from taichi_gaussian_rasterizer_amd import RasterConfig, _native as nv
from taichi_gaussian_rasterizer_amd.fused import is_frame_sparse_grad
from test_sparse_grad_gpu import PARAMS, _assert_same_training_state, check_half_in_view, half_in_view

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TOL = 1e-3  # what test_frame_sparse_gradients_match_dense holds two backward runs of one frame to
FACTOR = 3  # the kernel's largest error against the numpy float32 evaluation's: the device's exp / log / log1p / expm1
#             are 1-2 ulp functions of their own, numpy's are correctly rounded to ~0.5 ulp


# ------------------------------------------------------------------------------------------------- sampling rate
def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, -R @ eye
    return T


def camera_specs(count):
    """(T, projection, size, near, far): camera 0 is the identity pose with power-of-two numbers (the exact boundary
    rows below are its); the others stand on rings around the origin and differ in size, focal length and planes"""
    rng = np.random.default_rng(77)
    specs = [(np.eye(4), (32.0, 32.0, 32.0, 24.0), (64, 48), 0.5, 8.0)]
    for k in range(1, count):
        angle, radius = rng.uniform(0, 2 * np.pi), rng.uniform(3, 6)
        eye = (radius * np.cos(angle), rng.uniform(-1, 1), radius * np.sin(angle))
        w, h = int(rng.integers(40, 400)), int(rng.integers(30, 300))
        fx = float(rng.uniform(40, 400))
        specs.append((look_at(eye), (fx, fx * float(rng.uniform(0.8, 1.25)), w / 2 + float(rng.uniform(-3, 3)), h / 2),
                      (w, h), float(rng.uniform(0.2, 1.0)), float(rng.uniform(5, 30))))
    return specs[:count]


BOUNDARY = np.array([[0, 0, 0.5], [0, 0, 8.0], [2, 0, 1.0], [-2, 0, 1.0], [0, 3, 2.0],  # on camera 0's planes and lines
                     [2.0001, 0, 1.0], [0, 0, 0.4999], [0, 0, 8.001], [0, 0, -1.0],     # just outside, behind
                     [np.nan, 0, 1.0], [0, np.inf, 1.0], [0, 0, np.nan]], dtype=np.float32)


def point_pool(n=1000):
    """every 4th row one of the boundary rows, every 17th far from every camera, every 29th non-finite, the rest a
    cloud around the origin (inside some frusta, outside others, behind some cameras)"""
    rng = np.random.default_rng(5)
    pts = rng.normal(0, 1.5, (n, 3)).astype(np.float32)
    pts[::4] = BOUNDARY[np.arange(len(pts[::4])) % len(BOUNDARY)]
    pts[5::17] = (1e5, -1e5, 1e5)
    pts[7::29, 1] = np.nan
    pts[11::29, 2] = -np.inf
    return pts


POOL = point_pool()
SPECS = camera_specs(300)
TABLE = np.stack([ref.pack_camera(*spec, margin=0.5) for spec in SPECS])


@pytest.mark.parametrize("cameras", [0, 1, 2, 3, 63, 64, 65, 300])
def test_sampling_rate_is_bit_exact(cameras):
    """every N against every C; the kernel takes one camera per loop trip and stages no block of them, so there is no
    block size to straddle beyond these counts"""
    table = torch.from_numpy(TABLE[:cameras]).to(DEV)
    for n in (0, 1, 63, 64, 65, 257, 1000):
        pts = POOL[:n]
        rate, seen = gs.sampling_rate(torch.from_numpy(pts).to(DEV), table)
        want_rate, want_seen = ref.reference_sampling_rate(pts, TABLE[:cameras])
        assert rate.dtype == torch.float32 and seen.dtype == torch.int32 and rate.shape == seen.shape == (n,)
        assert np.array_equal(seen.cpu().numpy(), want_seen), (n, cameras)
        assert np.array_equal(rate.cpu().numpy().view(np.int32), want_rate.view(np.int32)), (n, cameras)
    if cameras >= 1:  # the hand-computed rows of camera 0 (test_mip_cabi.py) on the device, and the pool's coverage
        rate0, seen0 = gs.sampling_rate(torch.from_numpy(BOUNDARY).to(DEV), table[:1])
        assert seen0.tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
        assert rate0.tolist() == [64, 4, 32, 32, 16, 0, 0, 0, 0, 0, 0, 0]
    if cameras == 300:
        assert (want_seen == 0).sum() > 50 and (want_seen > 100).any() and len(np.unique(want_rate)) > 300
        finite = np.isfinite(POOL).all(1)
        assert (want_seen[~finite] == 0).all() and (want_rate[~finite] == 0).all()


def test_sampling_rate_from_camera_params_and_filter_3d():
    specs = SPECS[:7]
    cams = [gs.CameraParams(projection=torch.tensor(p, dtype=torch.float32, device=DEV),
                            T_camera_world=torch.tensor(T, dtype=torch.float32, device=DEV), near_plane=near,
                            far_plane=far, image_size=size) for T, p, size, near, far in specs]
    table = gs.pack_cameras(cams)
    assert table.device == DEV and tuple(table.shape) == (7, 24)
    want_table = np.stack([ref.pack_camera(*spec) for spec in specs])
    assert np.array_equal(table.cpu().numpy(), want_table)
    pts = torch.from_numpy(POOL).to(DEV)
    rate, seen = gs.sampling_rate(pts, cams)
    want_rate, want_seen = ref.reference_sampling_rate(POOL, want_table)
    assert np.array_equal(seen.cpu().numpy(), want_seen) and np.array_equal(rate.cpu().numpy(), want_rate)
    assert 0 < (want_seen == 0).sum() < len(POOL)

    size = gs.filter_3d(pts, table, variance=0.2)
    want = ref.reference_filter_3d(want_rate, want_seen, 0.2)
    assert size.shape == (len(POOL),) and size.dtype == torch.float32
    assert np.allclose(size.cpu().numpy(), want, rtol=2e-7, atol=0)
    unseen = torch.from_numpy(want_seen == 0).to(DEV)
    assert float(size[unseen].min()) == float(size[unseen].max()) == float(size[~unseen].max()) > 0
    # nothing seen: zeros; nothing at all: empty
    away = torch.full((9, 3), 1e6, device=DEV)
    assert gs.filter_3d(away, table).tolist() == [0.0] * 9
    assert gs.filter_3d(pts, table[:0]).abs().max().item() == 0.0
    assert gs.filter_3d(pts[:0], table).shape == (0,)


# ---------------------------------------------------------------------------------------------------- smoothing
def dev(*arrays, dtype=torch.float32):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype) for a in arrays]


def device_forward(l, a, f):
    tl, ta, tf = dev(l, a[:, None], f)
    out_l, out_a = gs.smooth3d(tl, ta, tf)
    assert out_l.shape == tl.shape and out_a.shape == ta.shape
    return out_l.cpu().numpy(), out_a.cpu().numpy()[:, 0]


def device_backward(l, a, f, gl, ga):
    tl, ta, tf, tgl, tga = dev(l, a[:, None], f, gl, ga[:, None])
    tl.requires_grad_(True)
    ta.requires_grad_(True)
    torch.autograd.backward(gs.smooth3d(tl, ta, tf), [tgl, tga])
    return tl.grad.cpu().numpy(), ta.grad.cpu().numpy()[:, 0]


def worst(got, truth, unit):
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.abs(got.astype(np.float64) - truth) / unit
    return float(np.nanmax(np.where(unit > 0, ratio, 0.0)))


@pytest.mark.parametrize("domain", ["moderate", "wide"])
def test_smooth3d_forward_against_float64(domain):
    """largest error in units of 2^-24 (|l| + |l'| + 1) and 2^-24 (|a| + |log c| + |a'| + 1): the kernel's is at most
    3 times that of the float32 numpy evaluation on the same 1000 rows.  N = 65 and N = 1 are the first 65 rows and row
    1 of them: the same bits as in the large call, so they are inside the same bound (one row alone has no meaningful
    largest error to take 3 times of).  Measured values: profiles/mip/accuracy.txt."""
    l, a, f = ref.smooth_inputs(1000, domain, 3)
    lp, ap, log_c = ref.smooth3d(l, a, f)
    lp32, ap32, _ = ref.smooth3d(l, a, f, np.float32)
    unit_l, unit_a = ref.forward_units(l.astype(np.float64), a.astype(np.float64), lp, ap, log_c)
    got_l, got_a = device_forward(l, a, f)
    assert np.isfinite(got_l).all() and np.isfinite(got_a).all()
    kernel = worst(got_l, lp, unit_l), worst(got_a, ap, unit_a)
    numpy32 = worst(lp32, lp, unit_l), worst(ap32, ap, unit_a)
    print(f"smooth3d forward, {domain}: kernel l' {kernel[0]:.2f} a' {kernel[1]:.2f} units; numpy float32 "
          f"l' {numpy32[0]:.2f} a' {numpy32[1]:.2f}")
    assert kernel[0] <= FACTOR * numpy32[0] and kernel[1] <= FACTOR * numpy32[1], (kernel, numpy32)
    for rows in (slice(0, 65), slice(1, 2)):
        assert f[1] != 0
        part_l, part_a = device_forward(l[rows], a[rows], f[rows])
        assert np.array_equal(part_l, got_l[rows]) and np.array_equal(part_a, got_a[rows])


@pytest.mark.parametrize("domain", ["moderate", "wide"])
def test_smooth3d_backward_against_float64(domain):
    """the dense backward against the analytic float64 gradients, in units of 2^-24 (|g_l| + 2 |g_a|) and 2^-24 |g_a|,
    by the rule of the forward test"""
    l, a, f = ref.smooth_inputs(1000, domain, 4)
    rng = np.random.default_rng(8)
    gl, ga = rng.standard_normal((1000, 3)).astype(np.float32), rng.standard_normal(1000).astype(np.float32)
    dl, da = ref.smooth3d_grad(l, a, f, gl, ga)
    dl32, da32 = ref.smooth3d_grad(l, a, f, gl, ga, np.float32)
    unit_l, unit_a = ref.backward_units(gl.astype(np.float64), ga.astype(np.float64))
    got_l, got_a = device_backward(l, a, f, gl, ga)
    assert np.isfinite(got_l).all() and np.isfinite(got_a).all()
    kernel = worst(got_l, dl, unit_l), worst(got_a, da, unit_a)
    numpy32 = worst(dl32, dl, unit_l), worst(da32, da, unit_a)
    print(f"smooth3d backward, {domain}: kernel dl {kernel[0]:.2f} da {kernel[1]:.2f} units; numpy float32 "
          f"dl {numpy32[0]:.2f} da {numpy32[1]:.2f}")
    assert kernel[0] <= FACTOR * numpy32[0] and kernel[1] <= FACTOR * numpy32[1], (kernel, numpy32)
    # one gradient alone: the other is taken as zero
    tl, ta, tf, tgl = dev(l, a[:, None], f, gl)
    tl.requires_grad_(True)
    ta.requires_grad_(True)
    out_l, _ = gs.smooth3d(tl, ta, tf)
    out_l.backward(tgl)
    only_l = ref.smooth3d_grad(l, a, f, gl, np.zeros_like(ga))
    assert worst(tl.grad.cpu().numpy(), only_l[0], unit_l) <= FACTOR * numpy32[0]
    assert float(ta.grad.abs().max()) == 0.0


def test_smooth3d_float64_gradcheck():
    l = torch.tensor([[0.3, -0.2, 0.1], [-3.0, 0.5, 2.0], [1.0, 1.5, -0.5], [-1.0, -2.0, 0.0], [0.2, 0.1, -0.1]],
                     dtype=torch.float64, device=DEV, requires_grad=True)
    a = torch.tensor([[0.5], [-1.5], [2.0], [-0.3], [4.0]], dtype=torch.float64, device=DEV, requires_grad=True)
    f = torch.tensor([0.0, 0.8, 0.05, 3.0, 1.0], dtype=torch.float64, device=DEV)  # f = 0; x > 1 in rows 1, 3 and 4
    assert bool(((f[:, None] * torch.exp(-l)) ** 2 > 1).any())
    assert torch.autograd.gradcheck(gs.smooth3d, (l, a, f), eps=1e-6, atol=1e-7, rtol=1e-6)
    out_l, out_a = gs.smooth3d(l, a, f)
    want = ref.smooth3d(l.detach().cpu().numpy(), a.detach().cpu().numpy()[:, 0], f.cpu().numpy())
    assert np.allclose(out_l.detach().cpu().numpy(), want[0], rtol=0, atol=1e-14)
    assert np.allclose(out_a.detach().cpu().numpy()[:, 0], want[1], rtol=0, atol=1e-13)
    with pytest.raises(TypeError, match="mixes"):
        gs.smooth3d(l, a.float(), f)
    with pytest.raises(TypeError, match="mixes"):
        gs.smooth3d(l.float(), a.float(), f)
    with pytest.raises(RuntimeError, match="HIP device"):
        gs.smooth3d(l, a, f.cpu())


def test_identity_and_rows_equal_dense():
    """f == 0 rows return inputs and gradients bit for bit, in the dense and in the row form; gs_smooth3d_bwd_rows on a
    random ascending subset equals the dense backward's rows bit for bit, also with one gradient missing"""
    n = 1000
    l, a, f = ref.smooth_inputs(n, "wide", 9)
    still = f == 0
    assert 100 < still.sum() < n
    rng = np.random.default_rng(10)
    gl, ga = rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    got_l, got_a = device_forward(l, a, f)
    assert np.array_equal(got_l[still], l[still]) and np.array_equal(got_a[still], a[still])
    assert not np.array_equal(got_l[~still], l[~still])
    dl, da = device_backward(l, a, f, gl, ga)
    assert np.array_equal(dl[still], gl[still]) and np.array_equal(da[still], ga[still])

    rows = np.sort(rng.choice(n, 377, replace=False))
    assert still[rows].any() and (~still[rows]).any()
    tl, ta, tf, tgl, tga = dev(l, a, f, gl[rows], ga[rows])
    trows = torch.from_numpy(rows).to(DEV)
    lib = nv.lib()
    for use_l, use_a in ((True, True), (True, False), (False, True)):
        out_l = torch.full((len(rows), 3), 7.0, device=DEV)
        out_a = torch.full((len(rows),), 7.0, device=DEV)
        nv.check(lib.gs_smooth3d_bwd_rows(n, len(rows), nv.ptr(trows), nv.ptr(tl), nv.ptr(ta), nv.ptr(tf),
                                          nv.ptr(tgl if use_l else None), nv.ptr(tga if use_a else None),
                                          nv.ptr(out_l), nv.ptr(out_a), nv.stream()), "gs_smooth3d_bwd_rows")
        dense_l, dense_a = device_backward(l, a, f, gl if use_l else np.zeros_like(gl), ga if use_a else np.zeros_like(ga))
        assert np.array_equal(out_l.cpu().numpy(), dense_l[rows]) and np.array_equal(out_a.cpu().numpy(), dense_a[rows])
        if use_l and use_a:
            at = still[rows]
            assert np.array_equal(out_l.cpu().numpy()[at], gl[rows][at])
            assert np.array_equal(out_a.cpu().numpy()[at], ga[rows][at])
    # a row index outside the table gives a zero row and reads nothing
    bad = trows.clone()
    bad[0], bad[-1] = -1, n
    nv.check(lib.gs_smooth3d_bwd_rows(n, len(rows), nv.ptr(bad), nv.ptr(tl), nv.ptr(ta), nv.ptr(tf), nv.ptr(tgl),
                                      nv.ptr(tga), nv.ptr(out_l), nv.ptr(out_a), nv.stream()), "gs_smooth3d_bwd_rows")
    assert out_l[[0, -1]].abs().max().item() == 0.0 and out_a[[0, -1]].abs().max().item() == 0.0


# ------------------------------------------------------------------------------------------ through the renderer
N_SCENE, SIZE = 1000, (96, 64)  # 2 000 Gaussians, half of them behind the camera


def _scene():
    g, cam = half_in_view(N_SCENE, SIZE, 1, 71)
    g = g.replace(feature=g.feature + 0.3 * torch.randn(g.feature.shape, generator=torch.Generator().manual_seed(2)))
    return g.to(DEV), cam.to(device=DEV)


def _filter(g, cams):
    size = gs.filter_3d(g.position, cams)
    assert float(size.min()) > 0
    return size


def _weights(cams, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return [torch.rand(c.image_size[1], c.image_size[0], 3, generator=gen).to(DEV) for c in cams]


def _check_sparse_leaves(a, rows, what):
    """all five leaf gradients are sparse over `rows` through one shared index tensor, recognised as a frame's own"""
    shared = a.position.grad._indices().data_ptr()
    for name in PARAMS:
        grad = getattr(a, name).grad
        assert grad.is_sparse and is_frame_sparse_grad(grad), (what, name)
        assert grad.shape == getattr(a, name).shape and grad._nnz() == rows.shape[0], (what, name)
        idx = grad._indices()
        assert idx.shape == (1, rows.shape[0]) and torch.equal(idx[0], rows), (what, name)
        assert idx.data_ptr() == shared, (what, name)


def _check_against_dense(sp, dn, rows, what):
    outside = torch.ones(sp.position.shape[0], dtype=torch.bool, device=DEV)
    outside[rows] = False
    assert bool(outside.any())
    for name in PARAMS:
        dense = getattr(dn, name).grad
        assert not dense.is_sparse and float(dense[outside].abs().max()) == 0.0, (what, name)
        assert float(dense[rows].abs().max()) > 0.0, (what, name)
        pu.assert_grad_close(getattr(sp, name).grad.to_dense(), dense, f"{what}: grad {name}", tol=TOL)


def test_sparse_gradients_stay_sparse_through_smooth3d(frame_path):
    g, cam = _scene()
    size = _filter(g, [cam])
    gi = _weights([cam])[0]
    runs = {}
    for sparse in (True, False):
        a = g.clone().requires_grad_(True)
        r = gs.render_gaussians(gs.smooth_gaussians(a, size), cam, RasterConfig(), use_sh=True, sparse_grad=sparse)
        (r.image * gi).sum().backward()
        runs[sparse] = (a, r)
    (sp, rs), (dn, rd) = runs[True], runs[False]
    assert torch.equal(rs.image, rd.image) and torch.equal(rs.points_in_view, rd.points_in_view)
    check_half_in_view(rs.points_in_view, 2 * N_SCENE)
    _check_sparse_leaves(sp, rs.points_in_view, "one frame")
    V = rs.points_in_view.shape[0]
    assert tuple(sp.log_scaling.grad._values().shape) == (V, 3) and tuple(sp.alpha_logit.grad._values().shape) == (V, 1)
    _check_against_dense(sp, dn, rs.points_in_view, "one frame")
    # the smoothing is in the graph: the same frame without it has other gradients
    plain = g.clone().requires_grad_(True)
    (gs.render_gaussians(plain, cam, RasterConfig(), use_sh=True, sparse_grad=True).image * gi).sum().backward()
    assert not torch.allclose(plain.log_scaling.grad.to_dense(), sp.log_scaling.grad.to_dense(), rtol=1e-2, atol=0)


def test_optimizer_step_from_the_smoothed_frame(frame_path):
    """a VisibilityAwareAdam step from the sparse gradients that came through smooth3d against the step from their dense
    form, as test_step_from_a_frame_gradient_equals_the_step_from_its_dense_form compares them"""
    from taichi_gaussian_rasterizer_amd.optim import VisibilityAwareAdam
    g, cam = _scene()
    N = 2 * N_SCENE
    size = _filter(g, [cam])
    kinds = (("position", 1e-3, "vector"), ("log_scaling", 1e-2, "vector"), ("rotation", 1e-2, "vector"),
             ("alpha_logit", 1e-1, "scalar"), ("feature", 1e-2, "scalar"))
    types = {k: t for k, _, t in kinds}
    sets = []
    for _ in range(2):
        params = {k: torch.nn.Parameter(v.clone()) for k, v in g.items()}
        sets.append((params, VisibilityAwareAdam([dict(params=[params[k]], name=k, lr=lr, type=t)
                                                  for k, lr, t in kinds])))
    (pd, od), (ps, os_) = sets
    cfg = RasterConfig(compute_visibility=True)
    target = _weights([cam], seed=2)[0]
    for step in range(2):
        os_.zero_grad()
        smoothed = gs.smooth_gaussians(type(g)(**ps, batch_size=(N,)), size)
        r = gs.render_gaussians(smoothed, cam, cfg, use_sh=True, sparse_grad=True)
        torch.nn.functional.l1_loss(r.image, target).backward()
        for k in ps:
            assert is_frame_sparse_grad(ps[k].grad), k
            pd[k].grad = ps[k].grad.to_dense()
        keep = r.point_visibility > 1e-8
        keep[::7] = False
        idx, w = r.points_in_view[keep], r.point_visibility[keep]
        assert 0 < idx.shape[0] < r.points_in_view.shape[0]
        od.step(idx, w)
        os_.step(idx, w)
        _assert_same_training_state((pd, od), (ps, os_), types, f"step {step}")
    assert not torch.equal(ps["log_scaling"].detach(), g.log_scaling)


def test_render_views_gradient_stays_sparse_through_smooth3d(frame_path):
    g, cam = _scene()
    move = torch.eye(4, device=DEV)
    move[0, 3], move[2, 3] = 0.6, 0.05  # far enough sideways to lose part of the scene
    cams = [cam, cam.scale_image(0.5), cam.transformed(move).scale_image(0.75)]
    assert len({c.image_size for c in cams}) == 3
    size = _filter(g, cams)
    weights = _weights(cams)
    runs = {}
    for sparse in (True, False):
        a = g.clone().requires_grad_(True)
        views = gs.render_views(gs.smooth_gaussians(a, size), cams, RasterConfig(), use_sh=True, sparse_grad=sparse)
        sum((r.image * w).sum() for r, w in zip(views, weights)).backward()
        runs[sparse] = (a, views.points_in_view)
    (sp, union), (dn, union_dense) = runs[True], runs[False]
    assert torch.equal(union, union_dense)
    assert torch.equal(union, torch.unique(torch.cat([v.points_in_view for v in views])))
    _check_sparse_leaves(sp, union, "render_views")
    _check_against_dense(sp, dn, union, "render_views")


def test_two_frames_over_one_smoothed_set_take_the_dense_fallback(frame_path):
    g, cam = _scene()
    move = torch.eye(4, device=DEV)
    move[0, 3] = 0.1
    cams = [cam, cam.transformed(move)]
    size = _filter(g, cams)
    weights = _weights(cams)
    runs = {}
    for sparse in (True, False):
        a = g.clone().requires_grad_(True)
        smoothed = gs.smooth_gaussians(a, size)
        sum((gs.render_gaussians(smoothed, c, RasterConfig(), use_sh=True, sparse_grad=sparse).image * w).sum()
            for c, w in zip(cams, weights)).backward()
        runs[sparse] = a
    sp, dn = runs[True], runs[False]
    for name in ("log_scaling", "alpha_logit"):  # autograd's sum of two frames' gradients is not a frame's: made dense
        assert not getattr(sp, name).grad.is_sparse, name
    assert sp.position.grad.is_sparse  # the frames' own gradients reach the other leaves as before
    for name in PARAMS:
        got = getattr(sp, name).grad
        pu.assert_grad_close(got.to_dense() if got.is_sparse else got, getattr(dn, name).grad, f"fallback: grad {name}",
                             tol=TOL)


def test_what_the_filter_is_for():
    """One Gaussian ten times smaller than a pixel of its training camera, smoothed with the filter that camera gives,
    rendered by that camera and by the same camera at half the resolution.

    What smoothing conserves is the Gaussian's mass in 3D, opacity * sqrt(det S): asserted to float32 rounding.  On the
    screen of its training camera the smoothed Gaussian is band-limited -- its projected variance is the filter's 0.2
    px^2 plus blur_cov, against 0.01 px^2 + blur_cov without smoothing -- and the summed image_weight of both renders
    equals the dense float64 renderer's on the smoothed parameters at the tolerance of the parity tests.  The summed
    image_weight itself is NOT the same at the two resolutions, with or without smoothing (blur_cov dilates every splat
    by a fixed number of pixels at either resolution, and the 3D normalisation divides by one more factor of the filter
    size than a 2D footprint has): the sums are printed, and asserted to differ without smoothing.  Measured on the
    MI355X, full against half resolution: 0.01935 and 0.01603 smoothed, 1.84695 and 1.79510 plain."""
    size, fx, depth = (64, 64), 64.0, 4.0
    cam = gs.CameraParams(projection=torch.tensor([fx, fx, 32.0, 32.0]), T_camera_world=torch.eye(4), near_plane=0.1,
                          far_plane=100.0, image_size=size).to(device=DEV)
    half = cam.scale_image(0.5)
    pixel = depth / fx  # world size of a pixel at the Gaussian
    one = gs.Gaussians3D(position=torch.tensor([[0.013, -0.021, depth]]),
                         log_scaling=torch.full((1, 3), math.log(pixel / 10)),
                         rotation=torch.tensor([[0.0, 0.0, 0.0, 1.0]]), alpha_logit=torch.tensor([[3.0]]),
                         feature=torch.ones(1, 3)).to(DEV)
    filt = gs.filter_3d(one.position, [cam])
    assert math.isclose(float(filt), math.sqrt(0.2) * pixel, rel_tol=1e-6)
    smooth = gs.smooth_gaussians(one, filt)
    mass = lambda g: float(torch.sigmoid(g.alpha_logit.double()).squeeze() * torch.exp(g.log_scaling.double().sum()))
    assert math.isclose(mass(smooth), mass(one), rel_tol=1e-5)
    cfg = RasterConfig()
    sums = {}
    for name, gaussians in (("smoothed", smooth), ("plain", one)):
        for res, camera in (("full", cam), ("half", half)):
            r = gs.render_gaussians(gaussians, camera, cfg, use_sh=False)
            assert r.points_in_view.shape[0] == 1
            _, alpha, _ = render_dense(r.gaussians2d.double(), r.point_depth.double(), gaussians.feature.double(),
                                       camera.image_size, cfg.clamp_max_alpha, cfg.alpha_threshold)
            pu.assert_pixels_close(r.image_weight, alpha, f"{name} {res}: image_weight")
            total, want = float(r.image_weight.double().sum()), float(alpha.sum())
            assert abs(total - want) <= pu.ATOL * alpha.numel() + pu.RTOL * want, (name, res, total, want)  # summed
            sums[name, res] = total
            variance = float(r.gaussians2d[0, 4] * r.gaussians2d[0, 5])
            if res == "full":
                expect = (0.2 + 0.01 if name == "smoothed" else 0.01) + cfg.blur_cov
                assert math.isclose(variance, expect, rel_tol=1e-3), (name, variance, expect)
    print("summed image_weight:", {f"{k[0]} {k[1]}": round(v, 5) for k, v in sums.items()})
    assert abs(sums["plain", "half"] - sums["plain", "full"]) > pu.RTOL * sums["plain", "full"] + pu.ATOL
    assert sums["smoothed", "full"] < sums["plain", "full"]  # the mass is spread, not added
