"""The weighted photometric-loss entry points without a GPU: symbols, host-side validation before any launch, the
Python argument errors of mask=, and the masked yardstick (tests/masked_loss_reference.py) checking itself."""
import ctypes

import pytest
import torch

import masked_loss_reference as mref
import ssim_reference as ref
from taichi_gaussian_rasterizer_amd import _native, losses

NAMES = ("gs_photo_loss_weighted_scratch_bytes", "gs_photo_loss_weighted_fwd", "gs_photo_loss_weighted_bwd",
         "gs_photo_loss_weighted_fwd_f64", "gs_photo_loss_weighted_bwd_f64")
P = ctypes.c_void_p(64)  # a non-NULL pointer that is never dereferenced: every call below stops on the host


def test_symbols_are_declared_exported_and_bound():
    import test_cabi
    declared = test_cabi.declared_functions()
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _native.SIGNATURES and hasattr(handle, name), name


def _fwd(lib, name, B=1, H=32, W=32, C=3, x=P, y=P, w=P, wst=None, ws=11, valid=0, scratch=P, nbytes=1 << 20,
         results=P):
    st = (H * W * C, W * C, C)
    wst = wst or (H * W, W, 1)
    return getattr(lib, name)(B, H, W, C, x, *st, y, *st, w, *wst, ws, 1.5, 1.0, 0.2, valid, None, None, scratch,
                              nbytes, results, None)


def _bwd(lib, name, B=1, H=32, W=32, C=3, x=P, y=P, w=P, wst=None, norm=P, ws=11, valid=0, saved=P, d_image=P):
    st = (H * W * C, W * C, C)
    wst = wst or (H * W, W, 1)
    return getattr(lib, name)(B, H, W, C, x, *st, y, *st, w, *wst, norm, ws, 1.5, valid, saved, None, None, 0.8, -0.2,
                              d_image, None)


@pytest.mark.parametrize("suffix", ["", "_f64"])
def test_forward_and_backward_validate_on_the_host(suffix):
    lib = _native.lib()
    f, b = "gs_photo_loss_weighted_fwd" + suffix, "gs_photo_loss_weighted_bwd" + suffix
    err = lib.gs_last_error
    # NULL buffers: everything the unweighted calls refuse, and the normalisers
    assert _fwd(lib, f, x=None) == -1 and b"NULL" in err()
    assert _fwd(lib, f, results=None) == -1 and b"NULL" in err()
    assert _fwd(lib, f, scratch=None) == -1 and b"NULL" in err()
    assert _bwd(lib, b, d_image=None) == -1 and b"NULL" in err()
    assert _bwd(lib, b, saved=None) == -1 and b"NULL" in err()
    assert _bwd(lib, b, norm=None) == -1 and b"normalisers" in err()
    assert _bwd(lib, b, norm=None, w=None) == -1 and b"normalisers" in err()
    # weight strides: pixel stride below 1, rows that overlap, batches that overlap
    for call in (_fwd, _bwd):
        name = f if call is _fwd else b
        assert call(lib, name, wst=(32 * 32, 32, 0)) == -1 and b"strides" in err() and b"weight" in err()
        assert call(lib, name, wst=(32 * 32, 31, 1)) == -1 and b"strides" in err()
        assert call(lib, name, wst=(32 * 32, 2 * 32 - 1, 2)) == -1 and b"strides" in err()
        assert call(lib, name, B=2, wst=(32 * 32 - 1, 32, 1)) == -1 and b"strides" in err()
        assert call(lib, name, B=2, wst=(-1, 32, 1)) == -1 and b"strides" in err()
    # accepted, so the call goes on to the next check and stops there: batch stride 0 (one mask for every batch entry),
    # a column view of a wider buffer, a NULL weight (the unweighted loss)
    for wst in ((0, 32, 1), (0, 80, 2), (40 * 80, 80, 1)):
        assert _fwd(lib, f, B=2, wst=wst, results=None) == -1 and b"NULL" in err() and b"strides" not in err()
        assert _bwd(lib, b, B=2, wst=wst, d_image=None) == -1 and b"NULL" in err() and b"strides" not in err()
    assert _fwd(lib, f, w=None, wst=(5, 5, 0), results=None) == -1 and b"results" in err()
    assert _bwd(lib, b, w=None, wst=(5, 5, 0), d_image=None) == -1 and b"d_image" in err()
    # what the unweighted calls check still holds
    assert _fwd(lib, f, C=0) == -1 and b"channels" in err()
    assert _fwd(lib, f, ws=10) == -1 and b"window_size" in err()
    assert _bwd(lib, b, W=5, valid=1) == -1 and b"valid" in err()
    # scratch: two more doubles per pixel tile than the unweighted call, whether or not a weight is given
    need = lib.gs_photo_loss_weighted_scratch_bytes(1, 32, 32, 3)
    assert need == lib.gs_photo_loss_scratch_bytes(1, 32, 32, 3) + 4 * 16
    assert _fwd(lib, f, nbytes=need - 1) == -4 and b"scratch" in err()
    assert _fwd(lib, f, w=None, nbytes=need - 1) == -4 and b"scratch" in err()
    # zero pixels: a no-op, whatever the pointers
    for shape in (dict(B=0), dict(H=0), dict(W=0)):
        assert _fwd(lib, f, x=None, y=None, w=None, results=None, scratch=None, nbytes=0, **shape) == 0
        assert _bwd(lib, b, x=None, y=None, w=None, norm=None, saved=None, d_image=None, **shape) == 0


def test_unweighted_scratch_query_is_unchanged():
    q, qw = _native.lib().gs_photo_loss_scratch_bytes, _native.lib().gs_photo_loss_weighted_scratch_bytes
    assert q(1, 16, 16, 1) == 16 and q(2, 37, 21, 5) == 2 * 3 * 2 * 3 * 16
    assert qw(2, 37, 21, 5) == q(2, 37, 21, 5) + 2 * 3 * 2 * 16 and qw(0, 64, 64, 3) == 0 and qw(1, 8, 8, 0) == 0


def test_python_argument_errors_come_before_any_launch():
    x, y = torch.rand(20, 24, 3), torch.rand(20, 24, 3)
    xb, yb = torch.rand(2, 20, 24, 3), torch.rand(2, 20, 24, 3)
    m = torch.rand(20, 24)
    for fn in (losses.ssim, losses.photometric_loss):
        # a good mask gets as far as the device check, in every accepted form
        for xi, yi, mi in ((x, y, m), (x, y, m > 0.5), (xb, yb, m), (xb, yb, torch.rand(2, 20, 24)),
                           (x.double(), y.double(), m.double()), (x, y, torch.rand(20, 40)[:, 3:27])):
            with pytest.raises(RuntimeError, match="HIP device"):
                fn(xi, yi, mask=mi)
        with pytest.raises(TypeError, match="mask"):
            fn(x, y, mask=m.numpy())
        with pytest.raises(TypeError, match="mask"):
            fn(x, y, mask=m.double())
        with pytest.raises(TypeError, match="mask"):
            fn(x.double(), y.double(), mask=m)
        with pytest.raises(TypeError, match="mask"):
            fn(x, y, mask=(m > 0.5).to(torch.uint8))
        for bad in (m[:-1], m.t(), m[None, None], torch.rand(20, 24, 3), torch.rand(2, 20, 24)):
            with pytest.raises(ValueError, match="mask"):
                fn(x, y, mask=bad)
        for bad in (torch.rand(3, 20, 24), torch.rand(2, 20), torch.rand(2, 24, 20)):
            with pytest.raises(ValueError, match="mask"):
                fn(xb, yb, mask=bad)
        with pytest.raises(ValueError, match="requires grad"):
            fn(x, y, mask=m.clone().requires_grad_(True))
        with pytest.raises(TypeError, match="mask on"):
            fn(x, y, mask=torch.empty(20, 24, device="meta"))
        # the image's own errors still come first
        with pytest.raises(ValueError, match="shape"):
            fn(x, y[:, :-1], mask=m)
    with pytest.raises(ValueError, match="reduction"):
        losses.ssim(x, y, reduction="none", mask=m)
    # mask is the last parameter: the positional calls of before keep their meaning
    with pytest.raises(ValueError, match="padding"):
        losses.photometric_loss(x, y, 0.2, 11, 1.5, 1.0, "reflect", False, m)
    with pytest.raises(ValueError, match="reduction"):
        losses.ssim(x, y, 11, 1.5, 1.0, "same", "sum", m)


# ------------------------------------------------------------------------------------------------ yardstick
@pytest.mark.parametrize("padding", ["same", "valid"])
def test_yardstick_float64_passes_gradcheck(padding):
    x, y = ref.make_pair("noise", (2, 13, 12, 2), seed=3)
    x, y = x.double(), y.double()
    x = torch.where((x - y).abs() < 1e-3, y + 1e-2, x).requires_grad_(True)
    kw = dict(eps=1e-6, check_grad_dtypes=True, check_undefined_grad=True)
    for mask in (mref.make_mask("random", x.shape), mref.make_mask("broadcast", x.shape)):
        assert torch.autograd.gradcheck(lambda t: mref.ssim(t, y, mask, padding=padding), (x,), **kw)
        assert torch.autograd.gradcheck(lambda t: mref.photometric_loss(t, y, mask, padding=padding), (x,), **kw)
        assert torch.autograd.gradcheck(lambda t: mref.photometric_loss(t, y, mask, window_size=5, padding=padding),
                                        (x,), **kw)


def test_yardstick_with_unit_weights_is_the_unmasked_yardstick():
    x, y = (t.double() for t in ref.make_pair("noise", (2, 30, 25, 3), seed=4))
    ones = torch.ones(2, 30, 25)
    for padding in ("same", "valid"):
        a, ga = mref.grad_of(mref.photometric_loss, x, y, ones, padding=padding)
        b, gb = ref.grad_of(ref.photometric_loss, x, y, padding=padding)
        assert torch.allclose(a, b, rtol=1e-13, atol=0) and torch.allclose(ga, gb, rtol=1e-12, atol=1e-18)
        assert torch.allclose(mref.ssim(x, y, ones, padding=padding), ref.ssim(x, y, padding=padding), rtol=1e-13)
    # scale invariance, an (H, W) mask for every batch entry, and an empty term
    m = mref.make_mask("broadcast", x.shape)
    a = mref.photometric_loss(x, y, m)
    assert torch.allclose(a, mref.photometric_loss(x, y, 3.0 * m), rtol=1e-13)
    assert torch.allclose(a, mref.photometric_loss(x, y, m.expand(2, 30, 25).clone()), rtol=1e-13)
    zero, g = mref.grad_of(mref.photometric_loss, x, y, torch.zeros(30, 25))
    L, M, S, Sv = mref.parts(x, y, torch.zeros(30, 25))
    assert float(zero) == 0.0 and not g.any() and bool(L.isnan()) and bool(M.isnan()) and float(S) == 0.0


def test_masks_are_seeded_float32_and_shaped_as_the_issue_says():
    shape = (2, 37, 21, 5)
    for kind in mref.MASKS:
        m, m2 = mref.make_mask(kind, shape), mref.make_mask(kind, shape)
        assert m.dtype == torch.float32 and torch.equal(m, m2) and float(m.min()) >= 0.0
        assert m.shape == ((37, 21) if kind == "broadcast" else (2, 37, 21))
    hole = mref.make_mask("hole", (40, 33, 3))
    assert not hole[10:30, 5:19].any() and int((hole == 0).sum()) == 20 * 14
    tile = mref.make_mask("one-tile", (40, 33, 3))
    assert bool((tile[16:32, :16] > 0).all()) and int((tile > 0).sum()) == 256
    one = mref.make_mask("single-pixel", (40, 33, 3))
    assert float(one.sum()) == 1.0 and float(one[20, 17]) == 1.0
