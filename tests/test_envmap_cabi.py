"""The environment-map entry points without a GPU: symbols, host-side validation before any launch, the scratch query,
the Python argument errors, and the yardstick (tests/envmap_reference.py) checking itself: against an explicit
per-pixel loop, against environment_directions, and against a map that is linear on every face."""
import ctypes

import pytest
import torch

import envmap_reference as ref
import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import _native, environment

NAMES = ("gs_envmap_scratch_bytes", "gs_envmap_fwd", "gs_envmap_bwd", "gs_envmap_fwd_f64", "gs_envmap_bwd_f64")
P = ctypes.c_void_p(64)  # a non-NULL pointer that is never dereferenced: every call below stops on the host


def test_symbols_are_declared_exported_and_bound():
    import test_cabi
    declared = test_cabi.declared_functions()
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _native.SIGNATURES and hasattr(handle, name), name
    assert "environment" in gs.__all__ and gs.environment is environment
    assert set(environment.__all__) == {"composite_environment", "sample_environment", "environment_directions",
                                        "constant_environment"}
    for name in environment.__all__:
        assert name in gs.__all__ and getattr(gs, name) is getattr(environment, name)
    assert "environment.composite_environment" in gs.render_gaussians.__doc__


def _fwd(lib, name, H=32, W=40, C=3, env=P, R=8, image=P, ist=None, weight=P, wst=None, proj=P, pose=P, out=P):
    ist = ist or (W * C, C)
    wst = wst or (W, 1)
    return getattr(lib, name)(H, W, C, env, R, image, *ist, weight, *wst, proj, pose, out, None)


def _bwd(lib, name, H=32, W=40, C=3, env=P, R=8, weight=P, wst=None, proj=P, pose=P, grad_out=P, d_weight=P, d_env=P,
         scratch=P, nbytes=1 << 40):
    wst = wst or (W, 1)
    return getattr(lib, name)(H, W, C, env, R, weight, *wst, proj, pose, grad_out, d_weight, d_env, scratch, nbytes,
                              None)


@pytest.mark.parametrize("suffix", ["", "_f64"])
def test_forward_and_backward_validate_on_the_host(suffix):
    lib = _native.lib()
    f, b = "gs_envmap_fwd" + suffix, "gs_envmap_bwd" + suffix
    err = lib.gs_last_error
    for call, name in ((_fwd, f), (_bwd, b)):
        for shape in (dict(H=0), dict(W=0), dict(H=-3)):
            assert call(lib, name, **shape) == -1 and b"empty" in err(), shape
        assert call(lib, name, R=0) == -1 and b"map edge" in err()
        for C in (0, 5, -1):
            assert call(lib, name, C=C) == -2 and b"channels" in err()
        assert call(lib, name, R=16385) == -2 and b"above 16384" in err()
        assert call(lib, name, H=1 << 16, W=1 << 15) == -2 and b"2^31" in err()
        assert call(lib, name, proj=None) == -1 and b"projection" in err()
        assert call(lib, name, pose=None) == -1 and b"T_camera_world" in err()
        assert call(lib, name, wst=(40, 0)) == -1 and b"strides of weight" in err()
        assert call(lib, name, wst=(39, 1)) == -1 and b"strides of weight" in err()
    # forward: NULL env / out, image without weight and the reverse, overlapping pixels or rows
    assert _fwd(lib, f, env=None) == -1 and b"NULL" in err()
    assert _fwd(lib, f, out=None) == -1 and b"NULL" in err()
    assert _fwd(lib, f, weight=None) == -1 and b"go together" in err()
    assert _fwd(lib, f, image=None) == -1 and b"go together" in err()
    assert _fwd(lib, f, ist=(40 * 3, 2)) == -1 and b"strides of image" in err()
    assert _fwd(lib, f, ist=(40 * 3 - 1, 3)) == -1 and b"strides of image" in err()
    # accepted: the sky alone, a channel slice of a 5-channel render, a weight column of a wider buffer, the largest map
    assert _fwd(lib, f, image=None, weight=None, out=None) == -1 and b"out" in err()
    assert _fwd(lib, f, ist=(40 * 5, 5), out=None) == -1 and b"out" in err()
    assert _fwd(lib, f, wst=(90, 2), out=None) == -1 and b"out" in err()
    assert _fwd(lib, f, R=16384, H=1, W=1, ist=(3, 3), wst=(1, 1), out=None) == -1 and b"out" in err()
    # backward
    assert _bwd(lib, b, grad_out=None) == -1 and b"grad_out" in err()
    assert _bwd(lib, b, d_weight=None, d_env=None) == -1 and b"no gradient" in err()
    assert _bwd(lib, b, weight=None) == -1 and b"d_weight without" in err()
    assert _bwd(lib, b, env=None) == -1 and b"d_weight without" in err()
    # a 64 x 130 image over a map of edge 2 cuts every texel's box into slices and needs scratch for their sums
    big = dict(H=130, W=64, R=2, wst=(64, 1))
    need = lib.gs_envmap_scratch_bytes(130, 64, 3, 2, int(bool(suffix)))
    assert need > 0
    assert _bwd(lib, b, scratch=None, **big) == -1 and b"scratch" in err()
    assert _bwd(lib, b, scratch=ctypes.c_void_p(68), **big) == -1 and b"aligned" in err()
    assert _bwd(lib, b, nbytes=need - 1, **big) == -4 and b"scratch" in err()
    # no d_env, no scratch: the call gets past validation only with real buffers, so it is not made here


def test_scratch_query():
    q = _native.lib().gs_envmap_scratch_bytes
    # one lane or one wave per texel, or enough texels to fill the chip: no scratch
    assert q(2048, 2048, 3, 2048, 0) == 0 and q(2048, 2048, 3, 512, 0) == 0 and q(1080, 1920, 3, 64, 0) == 0
    assert q(64, 64, 3, 64, 0) == 0 and q(64, 64, 3, 6, 0) == 0
    # 64 x 64 over an edge of 5: a box of (2 * 64 / 5 + 1)^2 = 707 pixels, one wave per texel, 707 / 256 = 2 slices
    assert q(64, 64, 3, 5, 0) == 6 * 25 * 2 * 3 * 4
    # 64 x 64 over 4 and 3: boxes of 1089 and 1907 pixels, four waves per texel, no room for a second slice
    assert q(64, 64, 3, 4, 0) == 0 and q(64, 64, 3, 3, 0) == 0 and q(64, 64, 3, 2, 0) == 6 * 4 * 4 * 3 * 4
    # 130 x 64 over an edge of 2: 131^2 = 17161 pixels, four waves per texel, 17161 / 1024 = 16 slices
    assert q(130, 64, 3, 2, 0) == 6 * 4 * 16 * 3 * 4 and q(130, 64, 4, 2, 1) == 6 * 4 * 16 * 4 * 8
    # 2048^2 over one texel a face: 64 slices at the most
    assert q(2048, 2048, 1, 1, 0) == 6 * 64 * 4
    assert q(0, 8, 3, 8, 0) == -1 and q(8, 8, 3, 0, 0) == -1 and q(8, 8, 5, 8, 0) == -2 and q(8, 8, 3, 16385, 0) == -2


def test_python_argument_errors_come_before_any_launch():
    fn = environment.composite_environment
    cam = ref.camera("seam", torch.float32)
    W, H = cam.image_size
    env, x, w = torch.rand(6, 4, 4, 3), torch.rand(H, W, 3), torch.rand(H, W)
    # good arguments get as far as the device check, in every accepted form
    for e, xi, wi, c in ((env, x, w, cam), (env, None, None, cam), (env.double(), x.double(), w.double(),
                                                                    ref.camera("seam", torch.float64)),
                         (env, torch.rand(H, W, 5)[..., 2:], torch.rand(H, W, 2)[..., 1], cam),
                         (torch.rand(6, 1, 1, 1), torch.rand(H, W, 1), w, cam)):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(e, xi, wi, c)
    with pytest.raises(RuntimeError, match="HIP device"):
        environment.sample_environment(env, cam)
    for bad in (torch.rand(5, 4, 4, 3), torch.rand(6, 4, 3, 3), torch.rand(6, 4, 4), torch.rand(6, 0, 0, 3)):
        with pytest.raises(ValueError, match="env must be"):
            fn(bad, None, None, cam)
    for C in (5, 0):
        with pytest.raises(ValueError, match="channels"):
            fn(torch.rand(6, 4, 4, C), None, None, cam)
    with pytest.raises(ValueError, match="go together"):
        fn(env, x, None, cam)
    with pytest.raises(ValueError, match="go together"):
        fn(env, None, w, cam)
    for bad in (torch.rand(H, W, 4), torch.rand(H, W), torch.rand(1, H, W, 3)):
        with pytest.raises(ValueError, match="image must be"):
            fn(env, bad, w, cam)
    with pytest.raises(ValueError, match="image_size"):
        fn(env, torch.rand(W, H, 3), torch.rand(W, H), cam)
    for bad in (w[:-1], w.t(), w[None], torch.rand(H, W, 3)):
        with pytest.raises(ValueError, match="image_weight"):
            fn(env, x, bad, cam)
    for e, xi, wi, c in ((env.double(), x, w, cam), (env, x.double(), w, cam), (env, x, w.double(), cam),
                         (env, x, w, ref.camera("seam", torch.float64)), (env.long(), x, w, cam),
                         (env, x, w > 0.5, cam)):
        with pytest.raises(TypeError, match="float32|float64"):
            fn(e, xi, wi, c)
    with pytest.raises(TypeError, match="must be a torch.Tensor"):
        fn(env.numpy(), x, w, cam)
    with pytest.raises(TypeError, match="image must be a torch.Tensor"):
        fn(env, x.numpy(), w, cam)
    with pytest.raises(TypeError, match="CameraParams"):
        fn(env, x, w, None)
    for kw in (dict(R=0), dict(R=2.0), dict(R=True)):
        with pytest.raises(ValueError, match="positive int"):
            environment.environment_directions(**kw)
    with pytest.raises(ValueError, match="positive int"):
        environment.constant_environment([1.0, 2.0], R=0)
    with pytest.raises(ValueError, match="channels"):
        environment.constant_environment([1.0] * 5, R=2)
    c = environment.constant_environment([0.25, 0.5, 0.75], R=3, dtype=torch.float64)
    assert c.shape == (6, 3, 3, 3) and c.is_contiguous() and bool((c == c[0, 0, 0]).all())
    assert c[5, 2, 1].tolist() == [0.25, 0.5, 0.75]


# ------------------------------------------------------------------------------------------------ yardstick
def test_the_cameras_see_the_faces_they_are_meant_to():
    seen = {name: ref.faces_seen(ref.camera(name)) for name in ref.CAMERAS}
    assert [len(seen[name]) for name in ("seam", "corner", "wide", "tele", "one", "small")] == [3, 4, 5, 2, 1, 1], seen
    for name, share in zip(("seam", "corner", "wide", "tele"), (0.0, 0.0004, 0.0002, 0.0)):
        left_out = 1.0 - float(ref.kept_pixels(ref.camera(name)).double().mean())
        assert left_out <= 0.01 and abs(left_out - share) < 5e-5, (name, left_out)
    for name in ("seam", "corner", "wide", "tele"):  # no kept pixel changes face between float32 and float64 directions
        cam = ref.camera(name)
        keep = ref.kept_pixels(cam)
        f64 = ref.lookup(ref.view_directions(cam, torch.float64), 8)[0]
        f32 = ref.lookup(ref.view_directions(ref.camera(name, torch.float32)), 8)[0]
        assert torch.equal(f64[keep], f32[keep]), name


@pytest.mark.parametrize("name,R,C", [("seam", 7, 3), ("small", 64, 1), ("corner", 2, 4), ("one", 1, 3)])
def test_yardstick_matches_the_explicit_loop(name, R, C):
    cam, env, image, weight, _, _ = ref.random_case(name, R, C, seed=3)
    if name == "corner":  # a 64 x 130 loop in Python is slow: the top-left 16 x 16 pixels see three faces
        cam = ref.make_camera((16, 16), (30, 30, 32, 65), cam.T_camera_world[:3, :3])
        image, weight = image[:16, :16], weight[:16, :16]
        assert len(ref.faces_seen(cam)) >= 2
    a = ref.composite_reference(env, image, weight, cam)
    b = ref.composite_loop(env, image, weight, cam)
    assert float((a - b).abs().max()) <= 1e-13
    assert float((ref.composite_reference(env, None, None, cam) - ref.composite_loop(env, None, None, cam)).abs().max()) \
        <= 1e-13


def test_translation_changes_nothing_in_the_yardstick():
    cam, env, image, weight, _, _ = ref.random_case("seam", 7, 3)
    moved = ref.camera("seam", translation=(5.0, 6.0, -7.0))
    assert torch.equal(ref.composite_reference(env, image, weight, cam), ref.composite_reference(env, image, weight, moved))


@pytest.mark.parametrize("R", [1, 2, 7, 64])
def test_environment_directions_round_trip(R):
    d = environment.environment_directions(R, dtype=torch.float64)
    assert d.shape == (6, R, R, 3)
    face, v, u = ref.lookup(d, R)
    f, j, i = torch.meshgrid(torch.arange(6), torch.arange(R), torch.arange(R), indexing="ij")
    assert torch.equal(face, f)
    assert torch.equal(v, j.double()) and torch.equal(u, i.double())


@pytest.mark.parametrize("name", ["seam", "corner", "wide", "tele"])
def test_a_map_linear_on_every_face_returns_each_pixels_face_coordinates(name):
    """a map holding its own (p, q) on every texel: bilinear interpolation reproduces a function linear in the face, so
    the yardstick returns each pixel's (p, q) at float64 rounding, for pixels at least half a texel inside their face
    (`tele` sees 0.03 of a face on either side of an edge: a finer map leaves it pixels that far inside)"""
    R = 512 if name == "tele" else 16
    cam = ref.camera(name)
    d = environment.environment_directions(R, dtype=torch.float64)
    env = torch.empty(6, R, R, 2, dtype=torch.float64)
    for face in range(6):
        first, second = ref.OTHERS[face // 2]
        env[face, :, :, 0], env[face, :, :, 1] = d[face, :, :, first], d[face, :, :, second]
    dirs = ref.view_directions(cam)
    mag = dirs.abs()
    axis = mag.argmax(-1)
    d_a = mag.gather(-1, axis[..., None])[..., 0]
    first = torch.tensor([o[0] for o in ref.OTHERS])[axis]
    second = torch.tensor([o[1] for o in ref.OTHERS])[axis]
    p = dirs.gather(-1, first[..., None])[..., 0] / d_a
    q = dirs.gather(-1, second[..., None])[..., 0] / d_a
    inside = (p.abs() <= 1 - 1.0 / R) & (q.abs() <= 1 - 1.0 / R)
    assert float(inside.double().mean()) > 0.5
    sky = ref.composite_reference(env, None, None, cam)
    assert float((sky[..., 0] - p)[inside].abs().max()) <= 1e-14
    assert float((sky[..., 1] - q)[inside].abs().max()) <= 1e-14
