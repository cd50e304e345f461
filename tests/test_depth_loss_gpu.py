"""depth.depth_prior_loss, pearson_depth_loss and fit_scale_shift on the MI355X against the float64 yardstick
(tests/depth_loss_reference.py) on the same inputs.

Bound (derived, not measured): a float32 output is a float64 result rounded once, so
|hip - yardstick| <= 2^-23 |yardstick| + 1e-12 (largest |value| of that output), for the loss, the parts,
fit_scale_shift and every element of d_depth, with no exclusions: test_depth_loss_cabi.py asserts that no case here has a
residual whose sign rounding could turn.  float64 inputs: 1e-12 of the output's largest magnitude, for the order of
the sums.  Modes that fit exactly through their pixels (depth_loss_reference.meaningful) are left out: their residuals
are rounding noise in any arithmetic.

Shapes: (1, 1), (1, 2), (3, 5) sit inside one wave; (67, 129) and (130, 257) spread one image over several workgroups
with a partial last run of pixels; (64, 64) is read 16 bytes at a time, the odd widths pixel by pixel; channel 0 of
an (H, W, 5) buffer and rows cut out of a taller buffer go in through their strides.  Rendering.median_depth is not
differentiable in the renderer, so the end-to-end test trains through Rendering.depth only.

`python tests/test_depth_loss_gpu.py [PATH]` writes the float32 errors of the HIP operator and of the float32 torch
composition (profiles/depth_loss/accuracy.txt)."""
import os
import sys

import pytest
import torch
from torch.autograd import gradcheck

import depth_loss_reference as ref
import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import _native, depth, scenes

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS32 = 2.0 ** -23


def _place(t, layout, dtype):
    """the tensor on the device in the layout: as made, channel 0 of a 5-channel buffer, rows 3.. of a taller buffer"""
    if t is None:
        return None
    t = t.to(device=DEV, dtype=dtype if t.is_floating_point() else None)
    if layout == "pixel5":
        buf = torch.full(t.shape + (5,), float("nan"), device=DEV, dtype=t.dtype)
        buf[..., 0] = t
        return buf[..., 0]
    if layout == "rows":
        H = t.shape[-2]
        buf = torch.full(t.shape[:-2] + (H + 7, t.shape[-1]), float("nan"), device=DEV, dtype=t.dtype)
        buf[..., 3:3 + H, :] = t
        return buf[..., 3:3 + H, :]
    return t


def _inputs(case, shape, layout="contiguous", dtype=torch.float32):
    d, p, m = ref.make_case(case, shape)
    return d, p, m, _place(d, layout, dtype), _place(p, layout, dtype), _place(m, layout, dtype)


def _run(kind, d, p, m, align, inverse):
    """loss, d_depth, parts and fit of the HIP operator"""
    x = d.detach().requires_grad_(True)
    if kind == "pearson":
        loss, parts, fit = depth.pearson_depth_loss(x, p, m, inverse), (), ()
    else:
        loss, parts = depth.depth_prior_loss(x, p, m, align, inverse, True)
        fit = depth.fit_scale_shift(d, p, m, align, inverse)
    loss.backward()
    return dict(loss=loss.detach(), grad=x.grad, parts=parts, fit=fit)


def _yardstick(kind, d, p, m, align, inverse):
    y = ref.evaluate(kind, d, p, m, align, inverse)
    y["fit"] = ref.fit_scale_shift(d, p, m, align, inverse) if kind == "l1" else ()
    return y


def _outputs(ours, y):
    """(name, hip, yardstick) of every output"""
    out = [("loss", ours["loss"], y["loss"]), ("d_depth", ours["grad"], y["grad"])]
    out += [(name, a, b) for name, a, b in zip(("L_b", "s_b", "t_b"), ours["parts"], y["parts"])]
    out += [(name, a, b) for name, a, b in zip(("scale", "shift"), ours["fit"], y["fit"])]
    return out


def _compare(ours, y, relative, floor, label):
    for name, a, b in _outputs(ours, y):
        a, b = a.detach().double().cpu().reshape(-1), b.reshape(-1)
        assert a.shape == b.shape, (label, name)
        nan = torch.isnan(b)
        assert torch.equal(torch.isnan(a), nan), (label, name)
        a, b = a[~nan], b[~nan]
        if b.numel() == 0:
            continue
        scale = float(b.abs().max())
        excess = ((a - b).abs() - relative * b.abs() - floor * scale)
        print(f"{label} {name}: max |error| {float((a - b).abs().max()):.3e}, magnitude {scale:.3e}")
        assert float(excess.max()) <= 0.0, (label, name, float((a - b).abs().max()), scale)


@pytest.mark.parametrize("case,shape,layout", ref.PARITY)
def test_float32_matches_the_yardstick_to_one_rounding(case, shape, layout):
    d, p, m, dd, pd, md = _inputs(case, shape, layout)
    for kind, align, inverse in ref.parity_modes(case, shape):
        ours = _run(kind, dd, pd, md, align, inverse)
        y = _yardstick(kind, d, p, m, align, inverse)
        _compare(ours, y, EPS32, 1e-12, f"{case} {shape} {layout} {kind} {align} inverse={inverse}")
        selected = ref.select(d, p, m, inverse)[3].reshape(d.shape)
        assert not bool(ours["grad"].cpu()[~selected].any())
        assert ours["grad"].shape == dd.shape and bool(torch.isfinite(ours["grad"]).all())


@pytest.mark.parametrize("case,shape", [(c, (67, 129)) for c in ref.CASES] +
                         [("plain", (3, 5)), ("holes", (64, 64)), ("offset", (130, 257)), ("plain", (3, 67, 129))])
def test_float64_matches_the_yardstick_to_summation_order(case, shape):
    d, p, m, dd, pd, md = _inputs(case, shape, dtype=torch.float64)
    for kind, align, inverse in ref.parity_modes(case, shape):
        ours = _run(kind, dd, pd, md, align, inverse)
        assert ours["grad"].dtype == torch.float64 and ours["loss"].dtype == torch.float64
        _compare(ours, _yardstick(kind, d, p, m, align, inverse), 0.0, 1e-12,
                 f"f64 {case} {shape} {kind} {align} inverse={inverse}")


def test_bool_and_shared_masks():
    d, p, m, dd, pd, md = _inputs("plain", (3, 67, 129))
    keep = m[0] > 0.4
    ours = _run("l1", dd, pd, keep.to(DEV), "affine", True)
    _compare(ours, _yardstick("l1", d, p, keep, "affine", True), EPS32, 1e-12, "bool (H, W) mask")
    ours = _run("pearson", dd, pd, md[1], "affine", False)
    _compare(ours, _yardstick("pearson", d, p, m[1], "affine", False), EPS32, 1e-12, "float (H, W) mask")


def test_the_shapes_cover_one_wave_and_several_workgroups_with_a_partial_run():
    q = _native.lib().gs_depth_loss_scratch_bytes
    waves = lambda shape: q(1, *shape[-2:]) // 64  # eight doubles a wave
    pixels = lambda shape: shape[-2] * shape[-1]
    shapes = {shape for _, shape, _ in ref.PARITY}
    assert any(waves(s) == 1 and pixels(s) <= 64 for s in shapes)
    assert any(waves(s) > depth.WORKGROUP_WAVES and pixels(s) % depth.WAVE_PIXELS != 0 for s in shapes)
    assert waves((67, 129)) == 34 and waves((130, 257)) == 131 and waves((3, 5)) == 1
    # 16-byte reads: (64, 64) qualifies, an odd width does not; both are compared above
    assert any(s[-1] % 4 == 0 for s in shapes) and any(s[-1] % 2 == 1 for s in shapes)


def test_holes_are_selected_out_and_outputs_stay_finite():
    d, p, m, dd, pd, md = _inputs("holes", (67, 129))
    assert not bool(torch.isfinite(p).all())
    for kind, align, inverse in ref.MODES:
        ours = _run(kind, dd, pd, md, align, inverse)
        selected = ref.select(d, p, m, inverse)[3].reshape(d.shape).to(DEV)
        assert bool(torch.isfinite(ours["loss"])) and bool(torch.isfinite(ours["grad"]).all())
        assert not bool(ours["grad"][~selected].any()) and bool(ours["grad"][selected].any())
        assert all(bool(torch.isfinite(v).all()) for v in ours["parts"] + tuple(ours["fit"]))
        filled = [t.to(DEV) for t in ref.fill_holes(d, p, m, inverse)]
        again = _run(kind, *filled, align, inverse)
        assert torch.equal(again["loss"], ours["loss"]) and torch.equal(again["grad"], ours["grad"])


def test_an_image_without_weight_adds_nothing():
    d, p, m, dd, pd, md = _inputs("empty", (67, 129))
    for align in ref.ALIGNS:
        ours = _run("l1", dd, pd, md, align, True)
        L, s, t = ours["parts"]
        assert bool(torch.isnan(L[1])) and bool(torch.isnan(s[1])) and bool(torch.isnan(t[1]))
        assert bool(torch.isnan(ours["fit"][0][1])) and bool(torch.isnan(ours["fit"][1][1]))
        assert not bool(ours["grad"][1].any()) and bool(ours["grad"][0].any()) and bool(ours["grad"][2].any())
        singles = [_run("l1", dd[b], pd[b], md[b], align, True) for b in (0, 2)]
        total = (singles[0]["loss"].double() + singles[1]["loss"].double()) / 3
        assert abs(float(ours["loss"].double() - total)) <= 2 * EPS32 * float(total)
        for b, one in zip((0, 2), singles):
            assert torch.equal(L[b], one["parts"][0][0]) and torch.equal(s[b], one["parts"][1][0])
            assert float((ours["grad"][b] * 3 - one["grad"]).abs().max()) <= 2 * EPS32 * float(one["grad"].abs().max())
    rho = _run("pearson", dd, pd, md, "affine", False)
    assert not bool(rho["grad"][1].any())
    all_zero = torch.zeros_like(md)
    nothing = _run("l1", dd, pd, all_zero, "affine", False)
    assert float(nothing["loss"]) == 0.0 and not bool(nothing["grad"].any())


def test_flat_prior_and_single_pixel_follow_the_degenerate_rules():
    d, p, m, dd, pd, md = _inputs("flat", (67, 129))
    ours = _run("l1", dd, pd, md, "affine", False)
    assert float(ours["parts"][1]) == 0.0 and float(ours["fit"][0]) == 0.0
    assert abs(float(ours["parts"][2]) - float(d.double().mean())) <= EPS32 * float(d.double().mean())
    flat = _run("pearson", dd, pd, md, "affine", False)
    assert float(flat["loss"]) == 1.0 and not bool(flat["grad"].any())
    zero = _run("l1", dd, torch.zeros_like(pd), md, "scale", False)
    assert float(zero["parts"][1]) == 0.0 and bool(torch.isfinite(zero["grad"]).all())
    d, p, m, dd, pd, md = _inputs("one", (67, 129))
    ours = _run("l1", dd, pd, md, "affine", False)
    assert float(ours["loss"]) == 0.0 and not bool(ours["grad"].any())
    assert float(ours["parts"][1]) == 0.0 and float(ours["parts"][2]) == float(d[m > 0])
    assert float(_run("pearson", dd, pd, md, "affine", True)["loss"]) == 1.0


def test_two_runs_repeat_bit_for_bit():
    for case, shape in (("plain", (130, 257)), ("holes", (3, 67, 129)), ("offset", (512, 515)), ("plain", (64, 64))):
        d, p, m, dd, pd, md = _inputs(case, shape)
        for kind, align, inverse in (("l1", "affine", True), ("l1", "scale", False), ("pearson", "affine", True)):
            a, b = _run(kind, dd, pd, md, align, inverse), _run(kind, dd, pd, md, align, inverse)
            assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["grad"], b["grad"])


def test_the_upstream_gradient_is_multiplied_in_before_the_rounding():
    d, p, m, dd, pd, md = _inputs("plain", (67, 129))
    x = dd.detach().requires_grad_(True)
    (depth.depth_prior_loss(x, pd, md, "affine", True) * 0.3).backward()
    y = ref.evaluate("l1", d, p, m, "affine", True)["grad"] * float(torch.tensor(0.3, dtype=torch.float32))
    err = (x.grad.double().cpu() - y).abs() - EPS32 * y.abs() - 1e-12 * float(y.abs().max())
    assert float(err.max()) <= 0.0


@pytest.mark.parametrize("kind,align", [("l1", "affine"), ("l1", "scale"), ("l1", "none"), ("pearson", "affine")])
@pytest.mark.parametrize("inverse", [False, True])
def test_gradcheck(kind, align, inverse):
    gen = torch.Generator().manual_seed(5)
    d = (1.0 + 5.0 * torch.rand(2, 9, 11, generator=gen, dtype=torch.float64)).to(DEV).requires_grad_(True)
    p = (0.3 * torch.rand(2, 9, 11, generator=gen, dtype=torch.float64) + 0.1).to(DEV)
    m = torch.where(torch.rand(2, 9, 11, generator=gen) < 0.7, torch.rand(2, 9, 11, generator=gen, dtype=torch.float64) + 0.1,
                    torch.zeros(2, 9, 11, dtype=torch.float64)).to(DEV)
    if kind == "pearson":
        fn = lambda x: depth.pearson_depth_loss(x, p, m, inverse)
    else:
        fn = lambda x: depth.depth_prior_loss(x, p, m, align, inverse)
    # |r| has kinks: the residuals of these inputs are ~1e-1, the probe 1e-6
    assert gradcheck(fn, (d,), eps=1e-6, atol=1e-7, rtol=1e-5, nondet_tol=0.0)


def test_a_render_trains_against_a_prior_end_to_end():
    g, camera = scenes.benchmark_scene(3000, (128, 96), sh_degree=3)
    g = g.to(DEV).requires_grad_(True)
    r = gs.render_gaussians(g, camera.to(device=DEV), gs.RasterConfig(), use_sh=True, render_depth=True)
    gen = torch.Generator().manual_seed(7)
    prior = (1.7 / r.depth.detach().clamp_min(0.1) + 0.2).cpu() + 0.02 * torch.randn(96, 128, generator=gen)
    mask = r.image_weight.detach() > 0.5
    assert 0 < int(mask.sum()) and r.depth.shape == (96, 128)
    loss = depth.depth_prior_loss(r.depth, prior.to(DEV), mask=mask, inverse=True)
    loss.backward()
    grad = g.position.grad
    grad = grad.to_dense() if grad is not None and grad.is_sparse else grad
    assert bool(torch.isfinite(loss.detach())) and float(loss.detach()) > 0
    assert grad is not None and bool(torch.isfinite(grad).all()) and bool(grad.any())


# ----------------------------------------------------------------------------------------------- the record
def write_accuracy(path):
    from taichi_gaussian_rasterizer_amd.benchmarks.bench_depth_loss import torch_depth_prior_loss, torch_pearson_loss
    lines = ["float32 accuracy of depth.depth_prior_loss / pearson_depth_loss on the MI355X (tests/test_depth_loss_gpu.py)",
             "max |error| against the float64 yardstick (tests/depth_loss_reference.py, on the CPU) on the same float32",
             "inputs: the HIP operator, the float32 torch composition on the device (textbook moments, the fit in the",
             "graph: benchmarks/bench_depth_loss.py), and the largest magnitude of the output.  The test's bound on the HIP",
             "operator is 2^-23 |value| + 1e-12 magnitude per element; the composition's column documents what it replaces",
             "and bounds nothing.", "",
             f"{'case':>7} {'shape':>13} {'mode':>16} {'output':>8} {'HIP':>10} {'torch f32':>10} {'magnitude':>10}"]
    for case, shape in [(c, (130, 257)) for c in ref.CASES] + [("plain", (512, 515)), ("holes", (64, 64))]:
        d, p, m, dd, pd, md = _inputs(case, shape)
        for kind, align, inverse in ref.parity_modes(case, shape):
            ours = _run(kind, dd, pd, md, align, inverse)
            y = ref.evaluate(kind, d, p, m, align, inverse)
            x = dd.detach().requires_grad_(True)
            theirs = torch_pearson_loss(x, pd, md, inverse) if kind == "pearson" else \
                torch_depth_prior_loss(x, pd, md, align, inverse)
            theirs.backward()
            mode = f"{kind if kind == 'pearson' else align}{' inverse' if inverse else ''}"
            for name, a, b, c in (("loss", ours["loss"], theirs.detach(), y["loss"]), ("d_depth", ours["grad"], x.grad, y["grad"])):
                err = [float((t.double().cpu() - c).abs().max()) for t in (a, b)]
                lines.append(f"{case:>7} {'x'.join(str(v) for v in d.shape):>13} {mode:>16} {name:>8} {err[0]:10.3e} "
                             f"{err[1]:10.3e} {float(c.abs().max()):10.3e}")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    write_accuracy(sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "depth_loss", "accuracy.txt"))
