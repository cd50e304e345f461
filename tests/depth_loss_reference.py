"""The float64 yardstick of taichi_gaussian_rasterizer_amd.depth: the definitions written plainly in torch on the CPU,
gradients from autograd (closed_form_gradient holds the formulas the kernels use, for the yardstick to check itself
against), and the generator of the named cases the tests share.

Selection is a torch.where in front of every use, so a pixel that is selected out adds nothing and gets a zero
gradient whatever it holds.  A case is float32 data; the yardstick computes on its float64 copy, i.e. on the same
float32 inputs the HIP operator reads.
"""
import functools

import torch

ALIGNS = ("affine", "scale", "none")
CASES = ("plain", "offset", "holes", "empty", "flat", "one")
FLAT = 1e-12
# (kind, align, inverse): the modes of the comparison
MODES = tuple(("l1", a, inv) for a in ALIGNS for inv in (False, True)) + (("pearson", "affine", False),
                                                                           ("pearson", "affine", True))


def _batched(t):
    return t if t.dim() == 3 else t[None]


def select(depth, prior, mask, inverse):
    """(w, p, x, selected) as (B, H, W) float64: zeros where a pixel is selected out"""
    d, q = _batched(depth).double(), _batched(prior).double()
    w = torch.ones_like(d) if mask is None else _batched(mask).double().expand_as(d)
    sel = (w > 0) & torch.isfinite(d) & torch.isfinite(q)
    if inverse:
        sel = sel & (d > 0)
    x = torch.where(sel, d, torch.ones_like(d))
    if inverse:
        x = 1.0 / x
    zero = torch.zeros_like(d)
    return torch.where(sel, w, zero), torch.where(sel, q, zero), torch.where(sel, x, zero), sel


def _sum(t):
    return t.sum((-2, -1))


def moments(w, p, x):
    W = _sum(w)
    safe = torch.where(W > 0, W, torch.ones_like(W))
    pm, xm = _sum(w * p) / safe, _sum(w * x) / safe
    dp, dx = p - pm[:, None, None], x - xm[:, None, None]
    # centred once more: a mean is rounded to its own magnitude (100 +- 0.01: 7e-15, which a factor rho / var_x = 90
    # makes 1e-12 of the Pearson gradient); what is left of sum w dp then is the rounding of the spread
    dp, dx = dp - (_sum(w * dp) / safe)[:, None, None], dx - (_sum(w * dx) / safe)[:, None, None]
    return dict(W=W, safe=safe, pm=pm, xm=xm, dp=dp, dx=dx, var_p=_sum(w * dp * dp), cov=_sum(w * dp * dx),
                var_x=_sum(w * dx * dx), spp=_sum(w * p * p), spx=_sum(w * p * x), sxx=_sum(w * x * x))


def _divide(num, den, bad):
    return torch.where(bad, torch.zeros_like(num), num / torch.where(bad, torch.ones_like(den), den))


def fit(m, align):
    """(s, t) per image from the moments, with the degenerate rules"""
    if align == "affine":
        s = _divide(m["cov"], m["var_p"], m["var_p"] <= FLAT * m["spp"])
        return s, m["xm"] - s * m["pm"]
    if align == "scale":
        return _divide(m["spx"], m["spp"], m["spp"] <= 0), torch.zeros_like(m["W"])
    assert align == "none", align
    return torch.ones_like(m["W"]), torch.zeros_like(m["W"])


def residuals(depth, prior, mask, align, inverse):
    w, p, x, sel = select(depth, prior, mask, inverse)
    m = moments(w, p, x)
    s, t = fit(m, align)
    return w, p, x, m, s, t, x - s[:, None, None] * p - t[:, None, None]


def depth_prior_loss(depth, prior, mask=None, align="affine", inverse=False):
    """loss, (L_b, s_b, t_b): the parts are NaN for an image without weight"""
    w, p, x, m, s, t, r = residuals(depth, prior, mask, align, inverse)
    L = _sum(w * r.abs()) / m["safe"]
    nan = torch.full_like(L, float("nan"))
    has = m["W"] > 0
    return L.mean(), tuple(torch.where(has, v.detach(), nan) for v in (L, s, t))


def pearson_depth_loss(depth, prior, mask=None, inverse=False):
    w, p, x, sel = select(depth, prior, mask, inverse)
    m = moments(w, p, x)
    flat = (m["W"] <= 0) | (m["var_p"] <= FLAT * m["spp"]) | (m["var_x"] <= FLAT * m["sxx"])
    one = torch.ones_like(m["W"])
    rho = _divide(m["cov"], torch.sqrt(torch.where(flat, one, m["var_p"]) * torch.where(flat, one, m["var_x"])), flat)
    return (1.0 - rho).mean()


def fit_scale_shift(depth, prior, mask=None, align="affine", inverse=False):
    w, p, x, m, s, t, r = residuals(depth, prior, mask, align, inverse)
    nan = torch.full_like(s, float("nan"))
    return torch.where(m["W"] > 0, s, nan), torch.where(m["W"] > 0, t, nan)


def evaluate(kind, depth, prior, mask, align, inverse):
    """dict(loss, grad (as depth), L, s, t) in float64; Pearson: no parts"""
    d = depth.double().detach().requires_grad_(True)
    if kind == "pearson":
        loss, parts = pearson_depth_loss(d, prior, mask, inverse), ()
    else:
        loss, parts = depth_prior_loss(d, prior, mask, align, inverse)
    grad, = torch.autograd.grad(loss, d)
    return dict(loss=loss.detach(), grad=grad, parts=parts)


def closed_form_gradient(kind, depth, prior, mask, align, inverse):
    """d loss / d depth by the formulas of the module docstring (what the kernels compute)"""
    with torch.no_grad():
        w, p, x, m, s, t, r = residuals(depth, prior, mask, align, inverse)
        B = w.shape[0]
        inv = (1.0 / m["safe"])[:, None, None]
        if kind == "pearson":
            flat = (m["W"] <= 0) | (m["var_p"] <= FLAT * m["spp"]) | (m["var_x"] <= FLAT * m["sxx"])
            one = torch.ones_like(m["W"])
            vp, vx = torch.where(flat, one, m["var_p"]), torch.where(flat, one, m["var_x"])
            root = torch.sqrt(vp * vx)
            rho = m["cov"] / root
            g = w * (m["dp"] / root[:, None, None] - (rho / vx)[:, None, None] * m["dx"])
            g = -torch.where(flat[:, None, None], torch.zeros_like(g), g)
        else:
            sg = torch.sign(r)
            A, Bs = _sum(w * sg * p), _sum(w * sg)
            bracket = sg
            if align == "affine":
                last = _divide(A - Bs * m["pm"], m["var_p"], m["var_p"] <= FLAT * m["spp"])
                bracket = sg - (Bs / m["safe"])[:, None, None] - last[:, None, None] * m["dp"]
            elif align == "scale":
                bracket = sg - _divide(A, m["spp"], m["spp"] <= 0)[:, None, None] * p
            g = w * inv * bracket
        if inverse:
            g = g * -(x * x)
        return (g / B).reshape(depth.shape)


# ------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def make_case(name, shape, seed=0):
    """(depth, prior, mask or None) in float32 for a shape (H, W) or (B, H, W); `empty` is a batch of 3 whatever the
    shape says.  Cached: treat the tensors as read-only."""
    gen = torch.Generator().manual_seed(1000 * CASES.index(name) + seed)
    shape = tuple(shape)
    if name == "empty":
        shape = (3,) + shape[-2:]
    rand = lambda: torch.rand(shape, generator=gen)
    randn = lambda: torch.randn(shape, generator=gen)
    depth = 1.0 + 5.0 * rand()
    prior = 0.2 * depth + 0.05 * randn()
    mask = None
    if name == "plain":
        mask = torch.where(rand() < 0.7, 0.05 + rand(), torch.zeros(shape))
    elif name == "offset":  # a far, thin scene: 100 +- 0.01 against a prior centred on 50, true scale about 0.019
        depth = 100.0 + 0.01 * randn()
        prior = 50.0 + (depth - 100.0) / 0.019 + 0.05 * randn()
    elif name == "holes":
        kind = torch.randint(0, 10, shape, generator=gen)
        mask = torch.where(kind < 4, torch.zeros(shape), 0.05 + rand())
        prior = torch.where(kind == 0, torch.full(shape, float("nan")), prior)
        prior = torch.where(kind == 1, torch.full(shape, float("inf")), prior)
        prior = torch.where(kind == 2, torch.full(shape, float("-inf")), prior)
        depth = torch.where(kind == 3, torch.zeros(shape), depth)
        depth = torch.where(kind == 4, torch.zeros(shape), depth)  # zeros that carry weight 1: inverse selects them out
        mask = torch.where(kind == 4, torch.ones(shape), mask)
    elif name == "empty":
        mask = torch.where(rand() < 0.7, 0.05 + rand(), torch.zeros(shape))
        mask[1] = 0.0
    elif name == "flat":
        prior = torch.full(shape, 2.5)
    elif name == "one":
        mask = torch.zeros(shape)
        mask.view(-1)[int(torch.randint(0, mask.numel(), (1,), generator=gen))] = 1.0
    else:
        raise KeyError(name)
    return depth.float(), prior.float(), None if mask is None else mask.float()


def fill_holes(depth, prior, mask, inverse):
    """the case with every selected-out pixel's depth and prior replaced by finite junk (its weight set to 0)"""
    w, p, x, sel = select(depth, prior, mask, inverse)
    sel = sel.reshape(depth.shape)
    junk = torch.full_like(depth, 7.25)
    keep = torch.ones_like(depth) if mask is None else _batched(mask).expand_as(_batched(depth)).reshape(depth.shape)
    return torch.where(sel, depth, junk), torch.where(sel, prior, -junk), torch.where(sel, keep, torch.zeros_like(keep))


def meaningful(kind, depth, prior, mask, align, inverse):
    """False where a fit passes exactly through its pixels -- two selected pixels under an affine fit or a correlation,
    one under a scale -- so that every residual (or the gradient of rho = +-1) is rounding noise with no sign to agree on"""
    count = select(depth, prior, mask, inverse)[3].sum((-2, -1))
    if kind == "pearson" or align == "affine":
        return not bool((count == 2).any())
    if align == "scale":
        return not bool((count == 1).any())
    return True


def smallest_residual_ratio(depth, prior, mask, align, inverse):
    """min over the weighted pixels with r != 0 of |r| / max |x| (inf if there is none)"""
    w, p, x, m, s, t, r = residuals(depth, prior, mask, align, inverse)
    live = (w > 0) & (r != 0)
    if not bool(live.any()):
        return float("inf")
    return float(r[live].abs().min() / x.abs().max())


# ---------------------------------------------------------------------------------- what the GPU comparison runs
SHAPES = ((1, 1), (1, 2), (3, 5), (64, 64), (67, 129), (130, 257), (512, 515), (3, 67, 129))
LAYOUTS = ("contiguous", "pixel5", "rows")  # as made; channel 0 of an (..., 5) buffer; rows cut out of a taller buffer
PARITY = tuple((case, shape, "contiguous") for shape in SHAPES for case in ("plain", "holes")) + \
    tuple((case, shape, "contiguous") for case in ("offset", "empty", "flat", "one") for shape in ((67, 129), (130, 257))) + \
    tuple((case, (67, 129), layout) for case in ("plain", "holes") for layout in LAYOUTS[1:])


def parity_modes(case, shape):
    """the modes of MODES that are meaningful on this case"""
    depth, prior, mask = make_case(case, shape)
    return tuple(mode for mode in MODES if meaningful(mode[0], depth, prior, mask, mode[1], mode[2]))
