"""The photometric-loss entry points without a GPU: symbols, the window, host-side validation before any launch, the
Python argument errors, and the yardstick (tests/ssim_reference.py) checking itself."""
import ctypes
import struct

import pytest
import torch

import ssim_reference as ref
from taichi_gaussian_rasterizer_amd import _native, losses

NAMES = ("gs_ssim_window", "gs_photo_loss_scratch_bytes", "gs_photo_loss_fwd", "gs_photo_loss_bwd",
         "gs_photo_loss_fwd_f64", "gs_photo_loss_bwd_f64")
P = ctypes.c_void_p(64)  # a non-NULL pointer that is never dereferenced: every call below stops on the host


def _window(ws, sigma):
    out = (ctypes.c_float * 16)()
    return _native.lib().gs_ssim_window(ws, sigma, out), list(out)[:max(ws, 0)]


def test_symbols_are_declared_exported_and_bound():
    import test_cabi
    declared = test_cabi.declared_functions()
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _native.SIGNATURES and hasattr(handle, name), name
    import taichi_gaussian_rasterizer_amd as gs
    assert "losses" in gs.__all__ and gs.losses is losses


def test_window_is_the_restatements_window_in_float32():
    rc, w = _window(11, 1.5)
    assert rc == 0
    expect = ref.window_1d(11, 1.5, torch.float32)
    assert [struct.pack("f", v) for v in w] == [struct.pack("f", float(v)) for v in expect]
    assert w == w[::-1]
    ulp = 2.0 ** -23
    assert abs(sum(float(v) for v in w) - 1.0) <= 11 * ulp
    assert torch.equal(losses.gaussian_window(11, 1.5), expect)
    for ws in (3, 5, 7, 9, 11, 13, 15):
        rc, w = _window(ws, 1.5)
        assert rc == 0 and len(w) == ws and w == w[::-1] and abs(sum(w) - 1.0) <= ws * ulp
        assert torch.equal(torch.tensor(w), ref.window_1d(ws, 1.5, torch.float32))
    lib = _native.lib()
    for ws in (0, 1, 4, 10, 16, 17, -3):
        assert _window(ws, 1.5)[0] == -1 and b"window_size" in lib.gs_last_error(), ws
    for sigma in (0.0, -1.0, float("nan")):
        assert _window(11, sigma)[0] == -1 and b"sigma" in lib.gs_last_error(), sigma
    assert lib.gs_ssim_window(11, 1.5, None) == -1 and b"NULL" in lib.gs_last_error()


def _fwd(lib, name="gs_photo_loss_fwd", B=1, H=32, W=32, C=3, x=P, xs=None, y=P, ys=None, ws=11, sigma=1.5,
         data_range=1.0, weight=0.2, valid=0, ssim_map=None, saved=None, scratch=P, nbytes=1 << 20, results=P):
    xs = xs or (H * W * C, W * C, C)
    ys = ys or (H * W * C, W * C, C)
    return getattr(lib, name)(B, H, W, C, x, *xs, y, *ys, ws, sigma, data_range, weight, valid, ssim_map, saved,
                              scratch, nbytes, results, None)


def _bwd(lib, name="gs_photo_loss_bwd", B=1, H=32, W=32, C=3, x=P, xs=None, y=P, ys=None, ws=11, sigma=1.5, valid=0,
         saved=P, upstream=None, grad=None, l1=0.8, ss=-0.2, d_image=P):
    xs = xs or (H * W * C, W * C, C)
    ys = ys or (H * W * C, W * C, C)
    return getattr(lib, name)(B, H, W, C, x, *xs, y, *ys, ws, sigma, valid, saved, upstream, grad, l1, ss, d_image,
                              None)


@pytest.mark.parametrize("suffix", ["", "_f64"])
def test_forward_and_backward_validate_on_the_host(suffix):
    lib = _native.lib()
    f, b = "gs_photo_loss_fwd" + suffix, "gs_photo_loss_bwd" + suffix
    err = lib.gs_last_error
    # NULL buffers
    assert _fwd(lib, f, x=None) == -1 and b"NULL" in err()
    assert _fwd(lib, f, y=None) == -1 and b"NULL" in err()
    assert _fwd(lib, f, results=None) == -1 and b"NULL" in err()
    assert _fwd(lib, f, scratch=None) == -1 and b"NULL" in err()
    assert _bwd(lib, b, x=None) == -1 and b"NULL" in err()
    assert _bwd(lib, b, d_image=None) == -1 and b"NULL" in err()
    assert _bwd(lib, b, saved=None) == -1 and b"NULL" in err()      # an SSIM term without the forward's maps
    # sizes, window, ranges
    assert _fwd(lib, f, C=0) == -1 and b"channels" in err()
    assert _bwd(lib, b, C=0) == -1 and b"channels" in err()
    assert _fwd(lib, f, H=-1) == -1
    assert _fwd(lib, f, ws=10) == -1 and b"window_size" in err()
    assert _bwd(lib, b, ws=17) == -1 and b"window_size" in err()
    assert _fwd(lib, f, sigma=0.0) == -1 and b"sigma" in err()
    assert _fwd(lib, f, data_range=0.0) == -1 and b"data_range" in err()
    assert _fwd(lib, f, weight=1.5) == -1 and b"ssim_weight" in err()
    assert _fwd(lib, f, H=10, valid=1) == -1 and b"valid" in err()
    assert _bwd(lib, b, W=5, valid=1) == -1 and b"valid" in err()
    assert _fwd(lib, f, H=10, W=11, valid=0, x=None) == -1 and b"NULL" in err()   # same padding takes any size
    # strides: pixel stride below the channel count, rows that overlap, batches that overlap
    assert _fwd(lib, f, xs=(32 * 32 * 3, 32 * 3, 2)) == -1 and b"strides" in err()
    assert _fwd(lib, f, ys=(32 * 32 * 3, 32 * 3 - 1, 3)) == -1 and b"strides" in err()
    assert _bwd(lib, b, xs=(32 * 32 * 3, 10, 3)) == -1 and b"strides" in err()
    assert _fwd(lib, f, B=2, xs=(32 * 32 * 3 - 1, 32 * 3, 3)) == -1 and b"strides" in err()
    assert _fwd(lib, f, xs=(0, 40 * 5, 5), x=None) == -1 and b"NULL" in err()     # a channel slice of a wider row: fine
    # scratch
    need = lib.gs_photo_loss_scratch_bytes(1, 32, 32, 3)
    assert _fwd(lib, f, nbytes=need - 1) == -4 and b"scratch" in err()
    # zero pixels: a no-op, whatever the pointers
    for shape in (dict(B=0), dict(H=0), dict(W=0)):
        assert _fwd(lib, f, x=None, y=None, results=None, scratch=None, nbytes=0, **shape) == 0
        assert _bwd(lib, b, x=None, y=None, saved=None, d_image=None, **shape) == 0
    with pytest.raises(ValueError):
        _native.check(_fwd(lib, f, C=0), f)


def test_scratch_query_grows_with_the_image():
    lib = _native.lib()
    q = lib.gs_photo_loss_scratch_bytes
    assert q(1, 16, 16, 1) >= 16
    assert q(1, 16, 16, 1) < q(1, 64, 64, 1) < q(1, 64, 64, 9) < q(3, 64, 64, 9)
    assert q(1, 2048, 2048, 3) < 1 << 20 and q(0, 64, 64, 3) == 0


def test_python_argument_errors_come_before_any_launch():
    x, y = torch.rand(20, 24, 3), torch.rand(20, 24, 3)
    for fn in (losses.ssim, losses.photometric_loss):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(x, y)
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(x.double(), y.double())
        with pytest.raises(TypeError):
            fn(x, y.double())
        with pytest.raises(TypeError):
            fn(x.double(), y)
        with pytest.raises(TypeError):
            fn(x, y.numpy())
        with pytest.raises(ValueError, match="shape"):
            fn(x, y[:, :-1])
        with pytest.raises(ValueError, match="expected"):
            fn(x[..., 0], y[..., 0])
        for ws in (10, 1, 17):
            with pytest.raises(ValueError, match="window_size"):
                fn(x, y, window_size=ws)
        with pytest.raises(ValueError, match="sigma"):
            fn(x, y, sigma=0.0)
        with pytest.raises(ValueError, match="data_range"):
            fn(x, y, data_range=0.0)
        with pytest.raises(ValueError, match="padding"):
            fn(x, y, padding="reflect")
        with pytest.raises(ValueError, match="valid"):
            fn(x[:8], y[:8], padding="valid")
        with pytest.raises(ValueError, match="requires grad"):
            fn(x, y.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="reduction"):
        losses.ssim(x, y, reduction="sum")
    for w in (-0.1, 1.1):
        with pytest.raises(ValueError, match="ssim_weight"):
            losses.photometric_loss(x, y, ssim_weight=w)


@pytest.mark.parametrize("kind", ["smooth", "flat", "near-equal"])
def test_yardstick_float32_is_ill_conditioned_where_the_bars_say(kind):
    """the accuracy bars of test_losses_gpu.py are fractions of the float32 restatement's error: that error has to be
    there on this torch build, or the bars are vacuous"""
    x, y = ref.make_pair(kind, (203, 157, 3))
    truth_map = ref.ssim_map(x.double(), y.double())
    _, truth_grad = ref.grad_of(ref.ssim, x.double(), y.double())
    map32 = ref.ssim_map(x, y)
    _, grad32 = ref.grad_of(ref.ssim, x, y)
    map_error = float((map32.double() - truth_map).abs().max())
    grad_error = ref.normwise(grad32.double() - truth_grad, truth_grad)
    print(f"{kind}: float32 restatement map error {map_error:.2e}, gradient error {grad_error:.2e}")
    assert map_error >= 1e-4 and grad_error >= 1e-4


def test_yardstick_float64_passes_gradcheck():
    x, y = ref.make_pair("noise", (13, 12, 2), seed=3)
    x, y = x.double(), y.double()
    x = torch.where((x - y).abs() < 1e-3, y + 1e-2, x).requires_grad_(True)
    kw = dict(eps=1e-6, check_grad_dtypes=True, check_undefined_grad=True)
    assert torch.autograd.gradcheck(lambda t: ref.ssim(t, y), (x,), **kw)
    assert torch.autograd.gradcheck(lambda t: ref.ssim(t, y, padding="valid"), (x,), **kw)
    assert torch.autograd.gradcheck(lambda t: ref.ssim_map(t, y, window_size=7), (x,), **kw)
    assert torch.autograd.gradcheck(lambda t: ref.photometric_loss(t, y), (x,), **kw)


def test_inputs_are_seeded_float32_and_signs_survive_the_conversion():
    for kind in ref.CLASSES:
        x, y = ref.make_pair(kind, (40, 30, 3))
        x2, y2 = ref.make_pair(kind, (40, 30, 3))
        assert x.dtype == torch.float32 and torch.equal(x, x2) and torch.equal(y, y2)
        assert torch.equal(torch.sign(x - y).double(), torch.sign(x.double() - y.double()))
