"""The bilateral-grid entry points without a GPU: symbols, host-side validation before any launch, the Python argument
errors, identity_grids and total_variation, and the yardstick (tests/bilagrid_reference.py) checking itself against an
explicit per-pixel loop of the formula."""
import ctypes

import pytest
import torch

import bilagrid_reference as ref
import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import _native, appearance

NAMES = ("gs_bilagrid_scratch_bytes", "gs_bilagrid_slice_fwd", "gs_bilagrid_slice_bwd", "gs_bilagrid_slice_fwd_f64",
         "gs_bilagrid_slice_bwd_f64")
P = ctypes.c_void_p(64)  # a non-NULL pointer that is never dereferenced: every call below stops on the host


def test_symbols_are_declared_exported_and_bound():
    import test_cabi
    declared = test_cabi.declared_functions()
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _native.SIGNATURES and hasattr(handle, name), name
    assert "appearance" in gs.__all__ and gs.appearance is appearance
    assert set(appearance.__all__) == {"slice_bilateral_grid", "identity_grids", "total_variation"}


def _fwd(lib, name, B=1, H=32, W=40, x=P, xst=None, guide=None, gst=None, grid=P, sizes=(8, 16, 16), gsb=None, out=P):
    xst = xst or (H * W * 3, W * 3, 3)
    gst = gst or (H * W, W, 1)
    gsb = 12 * sizes[0] * sizes[1] * sizes[2] if gsb is None else gsb
    return getattr(lib, name)(B, H, W, x, *xst, guide, *gst, grid, *sizes, gsb, out, None)


def _bwd(lib, name, B=1, H=32, W=40, x=P, xst=None, guide=None, gst=None, grid=P, sizes=(8, 16, 16), gsb=None,
         grad_out=P, d_image=P, d_guide=None, d_grid=P, scratch=P, nbytes=1 << 30):
    xst = xst or (H * W * 3, W * 3, 3)
    gst = gst or (H * W, W, 1)
    gsb = 12 * sizes[0] * sizes[1] * sizes[2] if gsb is None else gsb
    return getattr(lib, name)(B, H, W, x, *xst, guide, *gst, grid, *sizes, gsb, grad_out, d_image, d_guide, d_grid,
                              scratch, nbytes, None)


@pytest.mark.parametrize("suffix", ["", "_f64"])
def test_forward_and_backward_validate_on_the_host(suffix):
    lib = _native.lib()
    f, b = "gs_bilagrid_slice_fwd" + suffix, "gs_bilagrid_slice_bwd" + suffix
    err = lib.gs_last_error
    for call, name in ((_fwd, f), (_bwd, b)):
        # NULL buffers
        assert call(lib, name, x=None) == -1 and b"NULL" in err()
        assert call(lib, name, grid=None) == -1 and b"NULL" in err()
        # sizes that are not positive: an empty image is an error, so is an empty grid
        for shape in (dict(B=0), dict(H=0), dict(W=0), dict(H=-3), dict(sizes=(0, 16, 16)), dict(sizes=(8, 16, -1))):
            assert call(lib, name, **shape) == -1 and (b"empty" in err() or b"grid size" in err()), shape
        # strides: overlapping pixels, rows, batches; a guide likewise; grids that overlap
        assert call(lib, name, xst=(32 * 40 * 3, 40 * 3, 2)) == -1 and b"strides of image" in err()
        assert call(lib, name, xst=(32 * 40 * 3, 40 * 3 - 1, 3)) == -1 and b"strides of image" in err()
        assert call(lib, name, B=2, xst=(32 * 40 * 3 - 1, 40 * 3, 3)) == -1 and b"strides of image" in err()
        assert call(lib, name, guide=P, gst=(32 * 40, 40, 0)) == -1 and b"strides of guide" in err()
        assert call(lib, name, guide=P, gst=(32 * 40, 39, 1)) == -1 and b"strides of guide" in err()
        assert call(lib, name, B=2, gsb=12 * 8 * 16 * 16 - 1) == -1 and b"grid batch stride" in err()
        # unsupported: more levels than fit in LDS around one pixel (the message names the bound), a grid or an image
        # beyond the index range
        assert call(lib, name, sizes=(200, 2, 2)) == -2 and b"LDS" in err() and b"L <=" in err()
        assert call(lib, name, sizes=(16, 1 << 12, 1 << 12)) == -2 and b"2^31" in err()
        assert call(lib, name, W=(1 << 22) + 1, xst=(1 << 40, 1 << 30, 3)) == -2 and b"a side" in err()
    # accepted views stop at the next check: a channel slice of a 5-channel render, a guide column of a wider buffer
    assert _fwd(lib, f, xst=(32 * 40 * 5, 40 * 5, 5), out=None) == -1 and b"out" in err()
    assert _fwd(lib, f, guide=P, gst=(32 * 90, 90, 2), out=None) == -1 and b"out" in err()
    assert _fwd(lib, f, out=None) == -1 and b"NULL" in err()
    # every shape with Wg <= W, Hg <= H and L <= 16 is accepted, the finest grid an image can carry included
    for H, W, sizes in ((32, 40, (16, 32, 40)), (1, 1, (16, 1, 1)), (5, 6, (8, 5, 6)), (2048, 2048, (16, 16, 16))):
        assert _fwd(lib, f, H=H, W=W, sizes=sizes, out=None) == -1 and b"out" in err()
    # the backward's own buffers
    assert _bwd(lib, b, grad_out=None) == -1 and b"grad_out" in err()
    assert _bwd(lib, b, d_image=None, d_grid=None) == -1 and b"no gradient" in err()
    assert _bwd(lib, b, d_guide=P) == -1 and b"d_guide without a guide" in err()
    assert _bwd(lib, b, scratch=None) == -1 and b"scratch" in err()
    need = lib.gs_bilagrid_scratch_bytes(1, 32, 40, 8, 16, 16, int(bool(suffix)))
    assert need > 0
    assert _bwd(lib, b, nbytes=need - 1) == -4 and b"scratch" in err()


def test_scratch_query():
    q = _native.lib().gs_bilagrid_scratch_bytes
    # 2048^2 under (8, 16, 16): 32 x 32 pixel tiles touching at most 3 x 3 nodes, one float per level and channel
    assert q(1, 2048, 2048, 8, 16, 16, 0) == 64 * 64 * 3 * 3 * 8 * 12 * 4
    assert q(1, 2048, 2048, 1, 1, 1, 0) == 64 * 64 * 12 * 4
    assert q(2, 2048, 2048, 8, 16, 16, 1) == 2 * 2 * q(1, 2048, 2048, 8, 16, 16, 0)
    # a small image runs 8 x 8 tiles
    assert q(1, 37, 53, 1, 1, 1, 0) == 5 * 7 * 12 * 4
    assert q(0, 8, 8, 1, 1, 1, 0) == -1 and q(1, 8, 8, 0, 1, 1, 0) == -1
    assert q(1, 8, 8, 200, 2, 2, 0) == -2 and q(1, 8, 8, 100, 2, 2, 0) > 0 and q(1, 8, 8, 100, 2, 2, 1) == -2


def test_python_argument_errors_come_before_any_launch():
    fn = appearance.slice_bilateral_grid
    x, xb = torch.rand(20, 24, 3), torch.rand(2, 20, 24, 3)
    g, gb = appearance.identity_grids(1, 4, 3, 5)[0], appearance.identity_grids(2, 4, 3, 5)
    guide = torch.rand(20, 24)
    # good arguments get as far as the device check, in every accepted form
    for gi, xi, ui in ((g, x, None), (gb, xb, None), (g, x, guide), (gb, xb, torch.rand(2, 20, 24)),
                       (g.double(), x.double(), guide.double()), (gb[1], x, None),
                       (g, torch.rand(20, 24, 5)[..., 2:], None), (appearance.identity_grids(1, 1, 1, 1)[0], x, None)):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(gi, xi, ui)
    for bad in (torch.rand(20, 24, 4), torch.rand(20, 24), torch.rand(1, 2, 20, 24, 3)):
        with pytest.raises(ValueError, match="image must be"):
            fn(g, bad)
    for bad in (torch.rand(11, 4, 3, 5), torch.rand(12, 4, 3), gb, torch.rand(4, 3, 5, 12)):
        with pytest.raises(ValueError, match="grid must be"):
            fn(bad, x)
    with pytest.raises(ValueError, match="grid must be"):
        fn(g, xb)
    with pytest.raises(ValueError, match="3 grids for a batch of 2"):
        fn(appearance.identity_grids(3, 4, 3, 5), xb)
    with pytest.raises(ValueError, match="empty"):
        fn(g, torch.rand(0, 24, 3))
    with pytest.raises(ValueError, match="empty"):
        fn(torch.rand(12, 0, 3, 5), x)
    for gi, xi in ((g.double(), x), (g, x.double()), (g.half(), x.half().float()), (g.long(), x.long())):
        with pytest.raises(TypeError, match="both float32, or both float64"):
            fn(gi, xi)
    with pytest.raises(TypeError, match="must be a torch.Tensor"):
        fn(g.numpy(), x)
    with pytest.raises(TypeError, match="guide must be"):
        fn(g, x, guide.numpy())
    for bad in (guide[:-1], guide.t(), guide[None], torch.rand(20, 24, 3)):
        with pytest.raises(ValueError, match="guide"):
            fn(g, x, bad)
    with pytest.raises(ValueError, match="guide"):
        fn(gb, xb, guide)
    with pytest.raises(TypeError, match="guide is"):
        fn(g, x, guide.double())
    with pytest.raises(TypeError, match="guide on"):
        fn(g, x, torch.empty(20, 24, device="meta"))
    for kw in (dict(views=0), dict(views=1, L=0), dict(views=1, Hg=-1), dict(views=1, Wg=2.0), dict(views=True)):
        with pytest.raises(ValueError, match="positive int"):
            appearance.identity_grids(**kw)
    with pytest.raises(ValueError, match="total_variation"):
        appearance.total_variation(torch.rand(11, 2, 2, 2))


# ------------------------------------------------------------------------------------------------ yardstick
@pytest.mark.parametrize("with_guide", [False, True])
def test_yardstick_matches_the_explicit_loop(with_guide):
    grid, image, guide, upstream = ref.random_case((7, 9), (4, 3, 5), seed=18)  # luma clamped on both sides
    guide = guide if with_guide else None
    luma = ref.luma_of(image) if guide is None else guide
    assert bool((luma < 0).any()) and bool((luma > 1).any())  # some luma is clamped
    a = ref.grads_of(ref.slice_reference, grid, image, guide, upstream)
    b = ref.grads_of(ref.slice_loop, grid, image, guide, upstream)
    for name, s, t in zip(("value", "d_grid", "d_image", "d_guide"), a, b):
        if s is None:
            assert t is None and name == "d_guide" and not with_guide
            continue
        assert float((s - t).abs().max()) <= 1e-12, name
    if with_guide:  # a clamped guide passes no gradient
        assert not a[3][(guide < 0) | (guide > 1)].any() and bool(a[3].any())


def test_yardstick_on_a_single_node_is_one_affine_matrix():
    grid, image, _, _ = ref.random_case((7, 9), (1, 1, 1), seed=1)
    A = grid.view(3, 4)
    expected = image @ A[:, :3].t() + A[:, 3]
    assert torch.allclose(ref.slice_reference(grid, image), expected, rtol=0, atol=1e-14)
    assert float((ref.slice_loop(grid, image) - expected).abs().max()) <= 1e-14


def test_identity_grids_through_the_yardstick_return_the_image():
    grids = appearance.identity_grids(2, 4, 3, 5, dtype=torch.float64)
    assert grids.shape == (2, 12, 4, 3, 5) and grids.dtype == torch.float64
    assert bool((grids[:, (0, 5, 10)] == 1).all()) and float(grids.sum()) == 2 * 3 * 4 * 3 * 5
    assert appearance.identity_grids(1).shape == (1, 12, 8, 16, 16) and appearance.identity_grids(1).dtype == torch.float32
    _, image, guide, _ = ref.random_case((7, 9), (4, 3, 5), seed=2, batch=2)
    assert torch.allclose(ref.slice_reference(grids, image), image, rtol=0, atol=1e-15)
    assert torch.allclose(ref.slice_reference(grids, image, guide), image, rtol=0, atol=1e-15)


def test_total_variation():
    assert float(appearance.total_variation(appearance.identity_grids(3))) == 0.0
    assert float(appearance.total_variation(appearance.identity_grids(1, 1, 1, 1))) == 0.0
    # two levels of one node: level 0 holds zeros, level 1 holds c in channel c; the only neighbours are the 12 pairs
    # along L, so the value is mean(c^2) = (0 + 1 + 4 + ... + 121) / 12 = 506 / 12
    grid = torch.zeros(12, 2, 1, 1, dtype=torch.float64)
    grid[:, 1, 0, 0] = torch.arange(12, dtype=torch.float64)
    assert float(appearance.total_variation(grid)) == pytest.approx(506 / 12, rel=1e-15)
    # one step of 2 along Wg and one of 3 along Hg in channel 0 of a (1, 2, 2) grid: along Wg the differences are
    # (2, 2) in channel 0 and zero in the other 11 channels -> 8 / 24; along Hg (3, 3) -> 18 / 24
    grid = torch.zeros(12, 1, 2, 2, dtype=torch.float64)
    grid[0, 0] = torch.tensor([[0.0, 2.0], [3.0, 5.0]])
    assert float(appearance.total_variation(grid)) == pytest.approx(26 / 24, rel=1e-15)
    g = grid.clone().requires_grad_(True)
    appearance.total_variation(g).backward()
    assert g.grad is not None and bool(g.grad.any())
