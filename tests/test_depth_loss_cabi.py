"""The depth-loss entry points without a GPU: symbols, host-side validation before any launch, the scratch query, the
Python argument errors, and the yardstick (tests/depth_loss_reference.py) checking itself: autograd against the closed
forms, the invariances of the affine fit, holes against finite junk, and the condition on the inputs under which the
GPU comparison needs no outlier budget."""
import ctypes

import pytest
import torch

import depth_loss_reference as ref
import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import _native, depth

NAMES = ("gs_depth_loss_scratch_bytes", "gs_depth_loss_fwd", "gs_depth_loss_bwd", "gs_depth_loss_fwd_f64",
         "gs_depth_loss_bwd_f64")
P = ctypes.c_void_p(64)  # a non-NULL pointer that is never dereferenced: every call below stops on the host


def test_symbols_are_declared_exported_and_bound():
    import test_cabi
    declared = test_cabi.declared_functions()
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _native.SIGNATURES and hasattr(handle, name), name
    assert "depth" in gs.__all__ and gs.depth is depth
    assert set(depth.__all__) == {"depth_prior_loss", "pearson_depth_loss", "fit_scale_shift"}
    for name in depth.__all__:
        assert name in gs.__all__ and getattr(gs, name) is getattr(depth, name)


def _strides(B, H, W, st):
    return st or (H * W, W, 1)


def _fwd(lib, name, B=2, H=32, W=40, depth=P, dst=None, prior=P, pst=None, weight=P, wst=None, kind=0, align=0,
         inverse=0, results=P, stats=P, scratch=P, nbytes=1 << 40):
    return getattr(lib, name)(B, H, W, depth, *_strides(B, H, W, dst), prior, *_strides(B, H, W, pst), weight,
                              *_strides(B, H, W, wst), kind, align, inverse, results, stats, scratch, nbytes, None)


def _bwd(lib, name, B=2, H=32, W=40, depth=P, dst=None, prior=P, pst=None, weight=P, wst=None, kind=0, align=0,
         inverse=0, stats=P, g_loss=P, d_depth=P):
    return getattr(lib, name)(B, H, W, depth, *_strides(B, H, W, dst), prior, *_strides(B, H, W, pst), weight,
                              *_strides(B, H, W, wst), kind, align, inverse, stats, g_loss, d_depth, None)


@pytest.mark.parametrize("suffix", ["", "_f64"])
def test_forward_and_backward_validate_on_the_host(suffix):
    lib = _native.lib()
    f, b = "gs_depth_loss_fwd" + suffix, "gs_depth_loss_bwd" + suffix
    err = lib.gs_last_error
    for call, name in ((_fwd, f), (_bwd, b)):
        for shape in (dict(B=0), dict(H=0), dict(W=0), dict(H=-3)):
            assert call(lib, name, **shape) == -1 and b"empty" in err(), shape
        for shape in (dict(B=1, H=1 << 16, W=1 << 15), dict(B=2, H=1 << 15, W=1 << 15), dict(B=1 << 31, H=1, W=1)):
            assert call(lib, name, **shape) == -2 and b"2^31" in err(), shape
        assert call(lib, name, B=65536, H=1, W=1) == -2 and b"batch" in err()
        assert call(lib, name, depth=None) == -1 and b"NULL" in err()
        assert call(lib, name, prior=None) == -1 and b"NULL" in err()
        assert call(lib, name, stats=None) == -1 and b"NULL" in err()
        for which in ("dst", "pst", "wst"):
            what = {"dst": b"strides of depth", "pst": b"strides of prior", "wst": b"strides of weight"}[which]
            for bad in ((32 * 40, 40, 0), (32 * 40, 39, 1), (32 * 40 - 1, 40, 1), (32 * 80, 40, 2), (-1, 40, 1)):
                assert call(lib, name, **{which: bad}) == -1 and what in err(), (which, bad)
        assert call(lib, name, dst=(0, 40, 1)) == -1 and b"strides of depth" in err()  # only a weight is shared
        for mode in (dict(kind=3), dict(kind=-1), dict(align=3), dict(align=-1), dict(inverse=2)):
            assert call(lib, name, **mode) == -2 and b"unknown mode" in err(), mode
    assert _fwd(lib, f, results=None) == -1 and b"NULL" in err()
    assert _bwd(lib, b, d_depth=None) == -1 and b"NULL" in err()
    assert _bwd(lib, b, g_loss=None) == -1 and b"g_loss" in err()
    assert _bwd(lib, b, kind=2) == -2 and b"no backward" in err()
    need = lib.gs_depth_loss_scratch_bytes(2, 32, 40)
    assert need > 0
    assert _fwd(lib, f, scratch=None) == -1 and b"scratch" in err()
    assert _fwd(lib, f, scratch=ctypes.c_void_p(68)) == -1 and b"aligned" in err()
    assert _fwd(lib, f, nbytes=need - 1) == -4 and b"scratch" in err()
    # accepted, as far as the last check: no weight, one weight for the batch, a channel of a 5-channel buffer, rows of
    # a taller buffer, one image whatever its batch stride, every kind and align
    for ok in (dict(weight=None), dict(wst=(0, 40, 1)), dict(dst=(32 * 40 * 5, 40 * 5, 5)), dict(pst=(64 * 40, 40, 1)),
               dict(B=1, dst=(0, 40, 1)), dict(kind=1), dict(kind=2, align=2), dict(align=1, inverse=1)):
        assert _fwd(lib, f, scratch=None, **ok) == -1 and b"scratch" in err(), ok
        if ok.get("kind") != 2:
            assert _bwd(lib, b, g_loss=None, **ok) == -1 and b"g_loss" in err(), ok


def test_scratch_query():
    q = _native.lib().gs_depth_loss_scratch_bytes
    per_wave = 8 * 8  # eight doubles
    assert depth.WAVE_PIXELS == 256 and depth.WORKGROUP_WAVES == 4 and depth.STATS == 18
    # one wave's run is WAVE_PIXELS pixels of one image read pixel by pixel; the query sizes for that
    assert q(1, 1, 1) == per_wave and q(1, 3, 5) == per_wave and q(1, 16, 16) == per_wave and q(1, 1, 257) == 2 * per_wave
    assert q(3, 67, 129) == 3 * 34 * per_wave and q(1, 512, 515) == 1030 * per_wave and q(1, 130, 257) == 131 * per_wave
    assert q(1, 2048, 2048) == 2048 * 2048 // 4
    assert q(0, 8, 8) == -1 and q(1, 0, 8) == -1 and q(1, 8, -1) == -1
    assert q(1, 1 << 16, 1 << 15) == -2 and q(65536, 1, 1) == -2


def test_python_argument_errors_come_before_any_launch():
    H, W = 6, 7
    d, p = torch.rand(H, W) + 1, torch.rand(H, W)
    fns = (depth.depth_prior_loss, depth.pearson_depth_loss, depth.fit_scale_shift)
    # good arguments get as far as the device check, in every accepted form
    good = ((d, p, None), (d[None].expand(2, H, W), p[None].expand(2, H, W), None), (d, p, p > 0.5), (d, p, p),
            (torch.rand(2, H, W), torch.rand(2, H, W), p > 0.5), (torch.rand(2, H, W), torch.rand(2, H, W), torch.rand(2, H, W)),
            (torch.rand(H, W, 5)[..., 0], torch.rand(H, W, 5)[..., 2], None), (torch.rand(2 * H, W)[3:3 + H], p, None),
            (d.double(), p.double(), p.double()), (d.double(), p.double(), p > 0.5),
            (d.requires_grad_(True), p, None))
    for fn in fns:
        for x, y, m in good:
            with pytest.raises(RuntimeError, match="HIP device"):
                fn(x, y, m)
    for align in ref.ALIGNS:
        for inverse in (False, True):
            with pytest.raises(RuntimeError, match="HIP device"):
                depth.depth_prior_loss(d, p, None, align, inverse, True)
            with pytest.raises(RuntimeError, match="HIP device"):
                depth.fit_scale_shift(d, p, align=align, inverse=inverse)
    d = d.detach()
    for fn in fns:
        with pytest.raises(TypeError, match="depth must be a torch.Tensor"):
            fn(d.numpy(), p)
        with pytest.raises(TypeError, match="prior must be a torch.Tensor"):
            fn(d, None)
        for x, y in ((d, p[:-1]), (d, p.t()), (d[None], p)):
            with pytest.raises(ValueError, match="differ in shape"):
                fn(x, y)
        for bad in (torch.rand(7), torch.rand(1, 2, H, W)):
            with pytest.raises(ValueError, match=r"expected \(H, W\) or \(B, H, W\)"):
                fn(bad, bad.clone())
        for bad in (torch.rand(0, W), torch.rand(2, H, 0)):
            with pytest.raises(ValueError, match="empty"):
                fn(bad, bad.clone())
        for x, y in ((d.double(), p), (d, p.double()), (d.long(), p.long()), (d.half(), p)):
            with pytest.raises(TypeError, match="float32|float64"):
                fn(x, y)
        with pytest.raises(ValueError, match="prior requires grad"):
            fn(d, p.clone().requires_grad_(True))
        with pytest.raises(TypeError, match="inverse must be a bool"):
            fn(d, p, inverse=1)
        for bad in (torch.rand(W, H), torch.rand(1, H, W), torch.rand(H, W, 1)):
            with pytest.raises(ValueError, match="mask"):
                fn(d, p, bad)
        with pytest.raises(TypeError, match="mask"):
            fn(d, p, torch.rand(H, W).double())
        with pytest.raises(TypeError, match="mask must be a torch.Tensor"):
            fn(d, p, [[1.0]])
        with pytest.raises(ValueError, match="mask requires grad"):
            fn(d, p, torch.rand(H, W, requires_grad=True))
    for fn in (depth.depth_prior_loss, depth.fit_scale_shift):
        for bad in ("Affine", "shift", None, 0):
            with pytest.raises(ValueError, match="align"):
                fn(d, p, align=bad)
    with pytest.raises(TypeError, match="return_parts must be a bool"):
        depth.depth_prior_loss(d, p, return_parts=1)


# ------------------------------------------------------------------------------------------------ yardstick
SMALL = ((9, 11), (2, 9, 11))


@pytest.mark.parametrize("case", ref.CASES)
@pytest.mark.parametrize("shape", SMALL)
def test_autograd_equals_the_closed_forms(case, shape):
    d, p, m = ref.make_case(case, shape, seed=1)
    for kind, align, inverse in ref.MODES:
        if not ref.meaningful(kind, d, p, m, align, inverse):
            continue
        auto = ref.evaluate(kind, d, p, m, align, inverse)["grad"]
        closed = ref.closed_form_gradient(kind, d, p, m, align, inverse)
        assert bool(torch.isfinite(auto).all())
        assert float((auto - closed).abs().max()) <= 1e-13 * max(float(closed.abs().max()), 1e-300), (kind, align, inverse)
        selected = ref.select(d, p, m, inverse)[3].reshape(d.shape)
        assert not bool(auto[~selected].any())


@pytest.mark.parametrize("case", ["plain", "offset", "holes", "empty"])
def test_the_affine_fit_absorbs_scale_and_shift(case):
    d, p, m = ref.make_case(case, (9, 11), seed=2)
    for inverse in (False, True):
        base, parts = ref.depth_prior_loss(d, p, m, "affine", inverse)
        for a, b in ((2.0, 0.0), (-0.75, 3.0), (0.5, -4.0)):
            moved, _ = ref.depth_prior_loss(d, a * p.double() + b, m, "affine", inverse)
            assert abs(float(moved - base)) <= 1e-12 * max(abs(float(base)), 1.0), (a, b)
        g = ref.evaluate("l1", d, p, m, "affine", inverse)["grad"]
        w, q, x, sel = ref.select(d, p, m, inverse)
        g_x = ref.closed_form_gradient("l1", d, p, m, "affine", inverse)
        # in x (before the inverse's chain factor) the gradient is orthogonal to 1 and to the prior
        if inverse:
            g_x = torch.where(sel.reshape(d.shape), g_x / -(x * x).reshape(d.shape).clamp_min(1e-300), torch.zeros_like(g_x))
        scale = float(g_x.abs().sum())
        for b in range(sel.shape[0]):
            gb, qb = g_x.reshape(sel.shape)[b], q[b]
            assert abs(float(gb.sum())) <= 1e-13 * scale and abs(float((gb * qb).sum())) <= 1e-13 * scale * float(qb.abs().max())
        assert float((g - ref.closed_form_gradient("l1", d, p, m, "affine", inverse)).abs().max()) <= 1e-13 * float(g.abs().max())


@pytest.mark.parametrize("shape", SMALL)
def test_holes_equal_the_same_case_with_finite_junk(shape):
    d, p, m = ref.make_case("holes", shape, seed=3)
    assert not bool(torch.isfinite(p).all()) and bool((d == 0).any())
    for kind, align, inverse in ref.MODES:
        filled = ref.fill_holes(d, p, m, inverse)
        assert all(bool(torch.isfinite(t).all()) for t in filled)
        a = ref.evaluate(kind, d, p, m, align, inverse)
        b = ref.evaluate(kind, *filled, align, inverse)
        assert bool(torch.isfinite(a["loss"])) and torch.equal(a["loss"], b["loss"]) and torch.equal(a["grad"], b["grad"])
        for u, v in zip(a["parts"], b["parts"]):
            assert torch.equal(u, v)


def test_degenerate_rules():
    d, p, m = ref.make_case("empty", (9, 11))
    loss, (L, s, t) = ref.depth_prior_loss(d, p, m)
    assert bool(torch.isnan(L[1])) and bool(torch.isnan(s[1])) and bool(torch.isnan(t[1])) and bool(torch.isfinite(loss))
    singles = [ref.depth_prior_loss(d[b], p[b], m[b])[0] for b in (0, 2)]
    assert abs(float(loss - (singles[0] + singles[1]) / 3)) <= 1e-15
    assert not bool(ref.evaluate("l1", d, p, m, "affine", False)["grad"][1].any())
    d, p, m = ref.make_case("flat", (9, 11))
    loss, (L, s, t) = ref.depth_prior_loss(d, p, m)
    assert float(s) == 0.0 and abs(float(t) - float(d.double().mean())) <= 1e-14
    assert float(ref.pearson_depth_loss(d, p, m)) == 1.0
    d, p, m = ref.make_case("one", (9, 11))
    loss, (L, s, t) = ref.depth_prior_loss(d, p, m)
    assert float(loss) == 0.0 and float(s) == 0.0 and float(t) == float(d[m > 0])
    s1, t1 = ref.fit_scale_shift(d, p, m, "scale")
    assert float(s1) == pytest.approx(float(d[m > 0].double() / p[m > 0].double()), rel=1e-14) and float(t1) == 0.0
    zero = torch.zeros(9, 11)
    assert float(ref.fit_scale_shift(d, zero, None, "scale")[0]) == 0.0


@pytest.mark.parametrize("case,shape,layout", [c for c in ref.PARITY if c[2] == "contiguous"])
def test_no_residual_of_the_gpu_cases_is_rounding_noise(case, shape, layout):
    """the condition on the inputs: in the yardstick no weighted pixel has 0 < |r| < 1e-10 max |x|, for every case and
    mode the GPU comparison runs, so a pixel whose sign could legitimately differ does not exist there"""
    d, p, m = ref.make_case(case, shape)
    modes = ref.parity_modes(case, shape)
    assert ("l1", "none", False) in modes and (len(modes) == len(ref.MODES) or d.numel() <= 15 or case == "one")
    for kind, align, inverse in modes:
        if kind == "l1":
            assert ref.smallest_residual_ratio(d, p, m, align, inverse) >= 1e-10, (align, inverse)
