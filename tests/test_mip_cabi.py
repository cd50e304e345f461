"""The Mip-Splatting entry points without a GPU: they are exported and bound, every argument error is reported by the
host before any launch, the Python layer refuses bad arguments before it touches the device, the camera table holds the
hand-computed fields, and the references give the hand-computed answers."""
import ctypes
import math

import numpy as np
import pytest
import torch

import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import _native, mip

import mip_reference as ref

FAKE = 0x10000  # a non-NULL, 16-byte aligned address: validation fails before anything could read it
ENTRY_POINTS = {"gs_mip_sampling_rate": 7, "gs_smooth3d_fwd": 7, "gs_smooth3d_bwd": 9, "gs_smooth3d_bwd_rows": 11,
                "gs_smooth3d_fwd_f64": 7, "gs_smooth3d_bwd_f64": 9}
FUNCTIONS = ("filter_3d", "pack_cameras", "sampling_rate", "smooth3d", "smooth_gaussians")


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.lib()


def err(lib):
    return lib.gs_last_error()


def camera(width=64, height=48, fx=50.0, fy=40.0, near=0.5, far=20.0, T=None):
    T = torch.eye(4) if T is None else torch.as_tensor(T, dtype=torch.float32)
    return gs.CameraParams(projection=torch.tensor([fx, fy, width / 2, height / 2]), T_camera_world=T, near_plane=near,
                           far_plane=far, image_size=(width, height))


def test_exports_and_bindings(lib):
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name, args in ENTRY_POINTS.items():
        assert hasattr(handle, name), name
        assert len(_native.SIGNATURES[name][1]) == args, name
    assert _native.GS_MIP_CAMERA_FLOATS == 24 and _native.GS_MIP_CAMERAS_MAX == 65536
    assert gs.mip is mip and "mip" in gs.__all__
    for name in FUNCTIONS:
        assert name in gs.__all__ and name in mip.__all__ and getattr(gs, name) is getattr(mip, name), name


def test_sampling_rate_argument_errors(lib):
    rate = lib.gs_mip_sampling_rate
    assert rate(0, None, 0, None, None, None, None) == 0  # an empty call touches no pointer
    assert rate(0, None, 5, None, None, None, None) == 0
    assert rate(-1, FAKE, 1, FAKE, FAKE, FAKE, None) == -1 and b"rows" in err(lib)
    assert rate(2 ** 31, FAKE, 1, FAKE, FAKE, FAKE, None) == -1 and b"2^31" in err(lib)
    for cameras in (-1, 65537):
        assert rate(10, FAKE, cameras, FAKE, FAKE, FAKE, None) == -1 and b"cameras" in err(lib)
        assert rate(0, None, cameras, None, None, None, None) == -1  # also refused for an empty cloud
    for at, name in ((1, b"position"), (3, b"packed"), (4, b"rate"), (5, b"seen")):
        args = [10, FAKE, 2, FAKE, FAKE, FAKE, None]
        args[at] = None
        assert rate(*args) == -1 and b"NULL" in err(lib) and name in err(lib)
        args[at] = FAKE + 2
        assert rate(*args) == -1 and b"aligned" in err(lib) and name in err(lib)
    assert rate(10, FAKE, 0, None, None, FAKE, None) == -1 and b"rate" in err(lib)  # no cameras: packed may be NULL


@pytest.mark.parametrize("suffix, elem", [("", 4), ("_f64", 8)])
def test_smooth3d_argument_errors(lib, suffix, elem):
    fwd, bwd = getattr(lib, "gs_smooth3d_fwd" + suffix), getattr(lib, "gs_smooth3d_bwd" + suffix)
    assert fwd(0, None, None, None, None, None, None) == 0
    assert bwd(0, None, None, None, None, None, None, None, None) == 0
    for n in (-1, 2 ** 31):
        assert fwd(n, *[FAKE] * 5, None) == -1 and b"rows" in err(lib)
        assert bwd(n, *[FAKE] * 7, None) == -1 and b"rows" in err(lib)
    names = (b"log_scaling", b"alpha_logit", b"filter3d")
    for at, name in enumerate(names + (b"out_log_scaling", b"out_alpha_logit")):
        args = [FAKE] * 5
        args[at] = None
        assert fwd(10, *args, None) == -1 and b"NULL" in err(lib) and name in err(lib)
        args[at] = FAKE + elem // 2
        assert fwd(10, *args, None) == -1 and b"aligned" in err(lib) and name in err(lib)
    for at, name in enumerate(names + (b"grad_log_scaling", b"grad_alpha_logit", b"d_log_scaling", b"d_alpha_logit")):
        args = [FAKE] * 7
        args[at] = FAKE + elem // 2
        assert bwd(10, *args, None) == -1 and b"aligned" in err(lib) and name in err(lib)
        if at not in (3, 4):  # an incoming gradient may be NULL: it is zero
            args[at] = None
            assert bwd(10, *args, None) == -1 and b"NULL" in err(lib) and name in err(lib)


def test_smooth3d_rows_argument_errors(lib):
    rows = lib.gs_smooth3d_bwd_rows
    assert rows(0, 0, *[None] * 8, None) == 0
    assert rows(100, 0, *[None] * 8, None) == 0
    assert rows(-1, 5, *[FAKE] * 8, None) == -1 and b"rows" in err(lib)
    assert rows(2 ** 31, 5, *[FAKE] * 8, None) == -1 and b"2^31" in err(lib)
    assert rows(100, -1, *[FAKE] * 8, None) == -1 and b"gradient rows" in err(lib)
    assert rows(100, 2 ** 31, *[FAKE] * 8, None) == -1 and b"gradient rows" in err(lib)
    assert rows(0, 5, *[FAKE] * 8, None) == -1 and b"empty" in err(lib)
    names = (b"rows", b"log_scaling", b"alpha_logit", b"filter3d", b"grad_log_scaling", b"grad_alpha_logit",
             b"d_log_scaling", b"d_alpha_logit")
    for at, name in enumerate(names):
        args = [FAKE] * 8
        args[at] = FAKE + (4 if at == 0 else 2)
        assert rows(100, 5, *args, None) == -1 and b"aligned" in err(lib) and name in err(lib)
        if at not in (4, 5):
            args[at] = None
            assert rows(100, 5, *args, None) == -1 and b"NULL" in err(lib) and name in err(lib)


def test_python_refusals():
    l, a, f = torch.zeros(8, 3), torch.zeros(8, 1), torch.zeros(8)
    with pytest.raises(TypeError, match="Tensor"):
        gs.smooth3d(l.numpy(), a, f)
    with pytest.raises(TypeError, match="float32 or float64"):
        gs.smooth3d(l, a, f.int())
    for bad in (torch.zeros(8), torch.zeros(8, 2), torch.zeros(3, 8), torch.zeros(2, 8, 3)):
        with pytest.raises(ValueError, match="shape"):
            gs.smooth3d(bad, a, f)
    for bad in (torch.zeros(7), torch.zeros(8, 2), torch.zeros(8, 1, 1)):
        with pytest.raises(ValueError, match="shape"):
            gs.smooth3d(l, bad, f)
        with pytest.raises(ValueError, match="shape"):
            gs.smooth3d(l, a, bad)
    with pytest.raises(ValueError, match="requires grad"):
        gs.smooth3d(l, a, f.clone().requires_grad_())
    for args in ((l, a, f), (l.double(), a.double(), f.double()), (l, a.double(), f), (l, a.reshape(8), f.reshape(8, 1))):
        with pytest.raises(RuntimeError, match="HIP device"):  # well-formed, or mixed, but on the CPU: no fallback
            gs.smooth3d(*args)
    g = gs.Gaussians3D(position=l, log_scaling=l, rotation=torch.zeros(8, 4), alpha_logit=a, feature=torch.zeros(8, 3))
    with pytest.raises(TypeError, match="Gaussians3D"):
        gs.smooth_gaussians(dict(g.items()), f)
    with pytest.raises(RuntimeError, match="HIP device"):
        gs.smooth_gaussians(g, f)

    cams = [camera()]
    with pytest.raises(TypeError, match="Tensor"):
        gs.sampling_rate([[0.0, 0.0, 1.0]], cams)
    with pytest.raises(TypeError, match="float32"):
        gs.sampling_rate(l.double(), cams)
    for bad in (torch.zeros(8), torch.zeros(8, 2), torch.zeros(2, 8, 3)):
        with pytest.raises(ValueError, match="shape"):
            gs.sampling_rate(bad, cams)
    with pytest.raises(TypeError, match="sequence of CameraParams"):
        gs.sampling_rate(l, cams[0])
    with pytest.raises(TypeError, match="CameraParams"):
        gs.sampling_rate(l, [cams[0], "camera"])
    with pytest.raises(TypeError, match="float32"):
        gs.sampling_rate(l, torch.zeros(2, 24, dtype=torch.float64))
    for bad in (torch.zeros(24), torch.zeros(2, 23), torch.zeros(65537, 24)):
        with pytest.raises(ValueError, match="cameras|table"):
            gs.sampling_rate(l, bad)
    for margin in (-0.1, math.nan, "0.15"):
        with pytest.raises(ValueError, match="margin"):
            gs.pack_cameras(cams, margin=margin)
    for variance in (-1.0, math.inf):
        with pytest.raises(ValueError, match="variance"):
            gs.filter_3d(l, cams, variance=variance)
    for call in (gs.sampling_rate, gs.filter_3d):
        with pytest.raises(RuntimeError, match="HIP device"):
            call(l, cams)
        with pytest.raises(RuntimeError, match="HIP device"):
            call(torch.zeros(0, 3), gs.pack_cameras(cams))


def test_pack_cameras_fields():
    T = [[0.0, 1.0, 0.0, 0.25], [-1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 3.5], [0.0, 0.0, 0.0, 1.0]]
    cams = [camera(), camera(width=101, height=77, fx=33.5, fy=90.25, near=0.1, far=1000.0, T=T)]
    table = gs.pack_cameras(cams)
    assert table.dtype == torch.float32 and tuple(table.shape) == (2, 24) and table.device.type == "cpu"
    first, second = table.numpy()
    assert first[:12].tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    assert first[12:16].tolist() == [50, 40, 32, 24]
    f32 = np.float32
    assert first[16:20].tolist() == [f32(-0.15) * f32(64), (f32(1) + f32(0.15)) * f32(64), f32(-0.15) * f32(48),
                                     (f32(1) + f32(0.15)) * f32(48)]
    assert first[20:].tolist() == [0.5, 20, 50, 0]
    assert second[:12].tolist() == [0, 1, 0, 0.25, -1, 0, 0, -2, 0, 0, 1, 3.5]
    assert second[12:16].tolist() == [33.5, 90.25, 50.5, 38.5]
    assert second[16:20].tolist() == [f32(-0.15) * f32(101), f32(1.15) * f32(101), f32(-0.15) * f32(77),
                                      f32(1.15) * f32(77)]
    assert second[20:].tolist() == [f32(0.1), 1000, 90.25, 0]
    assert np.array_equal(second, ref.pack_camera(T, [33.5, 90.25, 50.5, 38.5], (101, 77), 0.1, 1000.0))
    wide = gs.pack_cameras(cams[:1], margin=0.5).numpy()[0]
    assert wide[16:20].tolist() == [-32, 96, -24, 72]
    assert tuple(gs.pack_cameras([]).shape) == (0, 24)


# ---- the sampling-rate reference against hand-computed cases
def test_reference_boundaries_are_inclusive():
    # identity pose, fx = fy = 32, centre (32, 24), 64 x 48, margin 0.5: u in [-32 z, 96 z], v in [-24 z, 72 z]
    table = ref.pack_camera(np.eye(4), [32, 32, 32, 24], (64, 48), 0.5, 8.0, margin=0.5)[None]
    points = np.array([[0, 0, 0.5],      # zc == near exactly
                       [0, 0, 8.0],      # zc == far exactly
                       [2, 0, 1.0],      # u = 32 * 2 + 32 = 96 = hi_x * 1: on the margin line exactly
                       [-2, 0, 1.0],     # u = -32 = lo_x
                       [0, 3, 2.0],      # v = 96 + 48 = 144 = 72 * 2
                       [2.0001, 0, 1.0],  # just outside
                       [0, 0, 0.4999], [0, 0, 8.001],
                       [0, 0, -1.0],     # behind the camera
                       [np.nan, 0, 1.0], [0, np.inf, 1.0], [0, 0, np.nan]], dtype=np.float32)
    rate, seen = ref.reference_sampling_rate(points, table)
    assert rate.dtype == np.float32 and seen.dtype == np.int32
    assert seen.tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert rate.tolist() == [64, 4, 32, 32, 16, 0, 0, 0, 0, 0, 0, 0]


def test_reference_largest_focal_over_depth_wins():
    near_cam = ref.pack_camera(np.eye(4), [100, 80, 50, 50], (100, 100), 0.1, 100.0)
    T_far = np.eye(4)
    T_far[2, 3] = 6.0  # the same point is 6 further away from this camera, whose focal length is 5 times larger
    far_cam = ref.pack_camera(T_far, [500, 400, 50, 50], (100, 100), 0.1, 100.0)
    point = np.array([[0, 0, 2.0]], dtype=np.float32)
    for table in (np.stack([near_cam, far_cam]), np.stack([far_cam, near_cam])):
        rate, seen = ref.reference_sampling_rate(point, table)
        assert seen.tolist() == [2] and rate[0] == np.float32(500) / np.float32(8)  # 62.5 > 100 / 2
    assert ref.reference_sampling_rate(point, near_cam[None])[0][0] == 50
    # the ratio is the correctly rounded float32 quotient
    third = ref.reference_sampling_rate(np.array([[0, 0, 3.0]], dtype=np.float32), near_cam[None])[0][0]
    assert third == np.float32(100) / np.float32(3) and third.dtype == np.float32
    empty = ref.reference_sampling_rate(point, np.zeros((0, 24), dtype=np.float32))
    assert empty[0].tolist() == [0] and empty[1].tolist() == [0]


def test_reference_operation_order():
    # xc = ((T00 px + T01 py) + T02 pz) + T03 in float32.  Row 0 = (1, 1, 1, 0), zc = px, fx = 1, cx = 0, a 1 x 1 image
    # without margin: valid needs u = xc <= zc.  For p = (1, 2^-24, 2^-24): ((1 + t) + t) = 1 = zc is valid, the other
    # association 1 + (t + t) = 1 + 2^-23 would not be
    T = np.array([[1, 1, 1, 0], [0, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1.0]])
    table = ref.pack_camera(T, [1, 1, 0, 0], (1, 1), 0.5, 2.0, margin=0.0)[None]
    tiny = np.float32(2.0 ** -24)
    point = np.array([[1, tiny, tiny]], dtype=np.float32)
    assert np.float32(1) + (tiny + tiny) > 1 and (np.float32(1) + tiny) + tiny == 1
    rate, seen = ref.reference_sampling_rate(point, table)
    assert seen.tolist() == [1] and rate.tolist() == [1]


def test_reference_filter_3d():
    rate = np.array([4, 0, 16, 0], dtype=np.float32)
    seen = np.array([1, 0, 3, 0], dtype=np.int32)
    size = ref.reference_filter_3d(rate, seen, variance=0.25)
    assert size.tolist() == [0.125, 0.125, 0.03125, 0.125]
    assert ref.reference_filter_3d(np.zeros(3, np.float32), np.zeros(3, np.int32)).tolist() == [0, 0, 0]


# ---- the smoothing reference
def test_reference_smoothing_hand_values():
    # l = 0, f = 1 on every axis: scale' = sqrt(2), c = 2^-3/2; opacity 1/2 -> opacity' = 2^-5/2
    lp, ap, log_c = ref.smooth3d(np.zeros((1, 3)), np.zeros(1), np.ones(1))
    assert np.allclose(lp, 0.5 * math.log(2), rtol=0, atol=1e-15)
    assert math.isclose(log_c[0], -1.5 * math.log(2), abs_tol=1e-15)
    o = 2.0 ** -2.5
    assert math.isclose(ap[0], math.log(o / (1 - o)), abs_tol=1e-14)
    # x > 1 on one axis, f == 0 in another row: bit for bit
    l = np.array([[-3.0, 0.5, 2.0], [0.3, -0.2, 0.1]])
    lp, ap, _ = ref.smooth3d(l, np.array([1.5, -0.7]), np.array([0.8, 0.0]))
    assert np.allclose(lp[0], 0.5 * np.log(np.exp(2 * l[0]) + 0.64), rtol=0, atol=1e-14)
    assert np.array_equal(lp[1], l[1]) and ap[1] == -0.7
    # the wide corners stay finite in both precisions
    corners = np.array([[-40.0, -40, -40], [40, 40, 40], [-40, 40, 0]])
    for f in (1e-12, 1e6):
        for a in (-40.0, 40.0):
            for dtype in (np.float64, np.float32):
                out = ref.smooth3d(corners, np.full(3, a), np.full(3, f), dtype)
                grads = ref.smooth3d_grad(corners, np.full(3, a), np.full(3, f), np.ones((3, 3)), np.ones(3), dtype)
                assert all(np.isfinite(v).all() for v in out + grads), (f, a, dtype)


def test_reference_gradients_match_autograd():
    rng = np.random.default_rng(5)
    n = 64
    l, a = rng.uniform(-2, 1, (n, 3)), rng.uniform(-3, 3, n)
    f = np.exp(rng.uniform(-3, 1, n))  # x on both sides of 1
    gl, ga = rng.standard_normal((n, 3)), rng.standard_normal(n)
    assert ((f[:, None] * np.exp(-l)) ** 2 > 1).any() and ((f[:, None] * np.exp(-l)) ** 2 < 1).any()
    tl, ta = torch.tensor(l, requires_grad=True), torch.tensor(a, requires_grad=True)
    out_l, out_a = ref.smooth3d_naive_torch(tl, ta, torch.tensor(f))
    lp, ap, _ = ref.smooth3d(l, a, f)
    assert np.allclose(out_l.detach().numpy(), lp, rtol=0, atol=1e-12)
    assert np.allclose(out_a.detach().numpy(), ap, rtol=0, atol=1e-11)
    (out_l * torch.tensor(gl)).sum().add((out_a * torch.tensor(ga)).sum()).backward()
    dl, da = ref.smooth3d_grad(l, a, f, gl, ga)
    assert np.allclose(tl.grad.numpy(), dl, rtol=1e-10, atol=1e-11)
    assert np.allclose(ta.grad.numpy(), da, rtol=1e-10, atol=1e-11)
    # f == 0: the gradients pass through bit for bit
    dl0, da0 = ref.smooth3d_grad(l, a, np.zeros(n), gl, ga)
    assert np.array_equal(dl0, gl) and np.array_equal(da0, ga)


def test_float32_evaluation_is_the_yardstick():
    """the float32 numpy evaluation of the stable forms stays within a few units of float64 on both domains, where the
    plainly written float32 composition does not (the reason the kernel uses these forms)"""
    for domain in ("moderate", "wide"):
        l, a, f = ref.smooth_inputs(20000, domain, 11)
        lp, ap, log_c = ref.smooth3d(l, a, f)
        lp32, ap32, _ = ref.smooth3d(l, a, f, np.float32)
        unit_l, unit_a = ref.forward_units(l.astype(np.float64), a.astype(np.float64), lp, ap, log_c)
        assert np.isfinite(lp32).all() and np.isfinite(ap32).all()
        assert (np.abs(lp32 - lp) / unit_l).max() < 4 and (np.abs(ap32 - ap) / unit_a[:]).max() < 12
    l, a, f = ref.smooth_inputs(20000, "moderate", 11)
    lp, ap, log_c = ref.smooth3d(l, a, f)
    _, unit_a = ref.forward_units(l.astype(np.float64), a.astype(np.float64), lp, ap, log_c)
    naive = ref.smooth3d_naive_torch(torch.tensor(l), torch.tensor(a), torch.tensor(f))[1].numpy()
    with np.errstate(invalid="ignore"):
        worst = np.nanmax(np.abs(naive.astype(np.float64) - ap) / unit_a)
    assert worst > 12 or not np.isfinite(naive).all()
