"""depth.depth_prior_loss and depth.pearson_depth_loss against the same losses composed in torch, and against plain
streaming.

Shapes: 2048 x 2048 and 1080 x 1920, each without a mask and with a float mask (a quarter of it zero), for
`affine` (align="affine", inverse=True, the common configuration) and `pearson` (inverse=True); `--depth_size H,W` runs
that one size instead.  The depth is a smooth surface between 2 and 10 with holes of 0 (1 % of the pixels), the prior
its inverse under a scale and a shift plus noise.  Per shape, forward (no autograd graph) and forward + backward of
  fused   the operator of depth.py
  torch   the loss as a trainer composes it today: select with torch.where, weighted means, the textbook moments,
          the fit, the L1 or the correlation, about 20 ops a direction, float32
  stream  passes that move the bytes the operation cannot avoid: a forward sweep reads depth and prior, and the mask if
          there is one (8 or 12 bytes per pixel), twice for the L1 loss (moments, then residuals) and once for Pearson;
          the backward reads them once more and writes the gradient (8 or 12, + 4)
all on the device, the three alternating round by round: `--warmup` calls, then `--iters` calls between two events;
`--rounds` rounds, median of the rounds, spread = largest minus smallest round.  fused_faster: the torch composition is
slower by more than either spread.  At these sizes the tensors stay in the 256 MiB last-level cache from call to call,
for all three paths alike.  One more row: a training iteration (render_gaussians(render_depth=True) + photometric
loss + backward, `--n` Gaussians at 1920 x 1080, or at the one size) alone, with 0.1 * depth_prior_loss(affine,
inverse, mask = image_weight > 0.5) added, and with the torch composition added.
--json PATH writes the record."""
from __future__ import annotations

import json

import torch

from .. import losses, scenes
from ..data_types import RasterConfig
from ..depth import depth_prior_loss, pearson_depth_loss
from ..renderer import render_gaussians
from .bench_bilagrid import _alternate, _summarise
from .util import FLAGS, make_parser

FLAGS.setdefault("rounds", dict(type=int, default=3))
FLAGS.setdefault("warmup", dict(type=int, default=3))
FLAGS.setdefault("depth_size", dict(type=str, default="", help="H,W: run this one size instead of the standard shapes"))
parse_args = make_parser(("device", "seed", "iters", "json", "rounds", "warmup", "depth_size", "n"), iters=20, n=200000)

SIZES = ((2048, 2048), (1080, 1920))
LOSSES = ("affine", "pearson")
SWEEPS = {"affine": 2, "pearson": 1}  # forward passes over the pixels


def sweep_bytes(pixels, masked):
    return (12 if masked else 8) * pixels


def forward_bytes(pixels, masked, loss):
    return SWEEPS[loss] * sweep_bytes(pixels, masked)


def backward_bytes(pixels, masked):
    return sweep_bytes(pixels, masked) + 4 * pixels


def _select(depth, prior, mask, inverse):
    valid = torch.isfinite(depth) & torch.isfinite(prior)
    if inverse:
        valid = valid & (depth > 0)
    w = valid.to(depth.dtype) if mask is None else torch.where(valid, mask.to(depth.dtype), torch.zeros_like(depth))
    x = torch.where(valid, depth, torch.ones_like(depth))
    x = 1.0 / x if inverse else x
    return w, torch.where(valid, prior, torch.zeros_like(prior)), torch.where(valid, x, torch.zeros_like(x))


def _mean(t, W):
    return t.sum((-2, -1)) / W


def _each(v):
    return v[..., None, None]


def torch_depth_prior_loss(depth, prior, mask=None, align="affine", inverse=True):
    """the loss as a trainer composes it, in the dtype of its inputs: textbook moments E[px] - E[p] E[x], the fit
    attached to the graph; (H, W) or (B, H, W)"""
    w, p, x = _select(depth, prior, mask, inverse)
    W = w.sum((-2, -1)).clamp_min(1e-12)
    s, t = torch.ones_like(W), torch.zeros_like(W)
    if align == "affine":
        pm, xm = _mean(w * p, W), _mean(w * x, W)
        s = (_mean(w * p * x, W) - pm * xm) / (_mean(w * p * p, W) - pm * pm)
        t = xm - s * pm
    elif align == "scale":
        s = (w * p * x).sum((-2, -1)) / (w * p * p).sum((-2, -1))
    return _mean(w * (x - _each(s) * p - _each(t)).abs(), W).mean()


def torch_pearson_loss(depth, prior, mask=None, inverse=True):
    w, p, x = _select(depth, prior, mask, inverse)
    W = w.sum((-2, -1)).clamp_min(1e-12)
    pm, xm = _mean(w * p, W), _mean(w * x, W)
    var_p, var_x = _mean(w * p * p, W) - pm * pm, _mean(w * x * x, W) - xm * xm
    return (1.0 - (_mean(w * p * x, W) - pm * xm) / torch.sqrt(var_p * var_x)).mean()


def fused_affine(depth, prior, mask=None):
    return depth_prior_loss(depth, prior, mask, "affine", True)


def fused_pearson(depth, prior, mask=None):
    return pearson_depth_loss(depth, prior, mask, True)


PATHS = {"affine": (fused_affine, torch_depth_prior_loss), "pearson": (fused_pearson, torch_pearson_loss)}


def make_inputs(H, W, gen):
    """(depth, prior, mask): a smooth surface with holes, its disparity under a scale and a shift plus noise"""
    u = ((torch.arange(W) + 0.5) / W).view(1, W)
    v = ((torch.arange(H) + 0.5) / H).view(H, 1)
    depth = 6.0 + 3.0 * torch.sin(6.283185 * (1.5 * u + 0.7 * v)) * torch.cos(6.283185 * (0.8 * v - 0.3 * u)) + \
        0.5 * torch.rand(H, W, generator=gen)
    prior = 3.0 / depth + 0.2 + 0.01 * torch.randn(H, W, generator=gen)
    depth = torch.where(torch.rand(H, W, generator=gen) < 0.01, torch.zeros(H, W), depth)
    mask = torch.where(torch.rand(H, W, generator=gen) < 0.25, torch.zeros(H, W), torch.rand(H, W, generator=gen))
    return depth, prior, mask


def bench_case(args, shape, masked, loss):
    H, W = shape
    dev = args.device
    gen = torch.Generator().manual_seed(args.seed)
    depth, prior, mask = (t.to(dev) for t in make_inputs(H, W, gen))
    mask = mask if masked else None
    fused, composed = PATHS[loss]
    out = torch.empty_like(depth)

    def forward(fn):
        with torch.no_grad():
            fn(depth, prior, mask)

    def forward_backward(fn):
        fn(depth.detach().requires_grad_(True), prior, mask).backward()

    def stream_sweep():
        depth.sum()
        prior.sum()
        if masked:
            mask.sum()

    def stream_forward():
        for _ in range(SWEEPS[loss]):
            stream_sweep()

    def stream_both():
        stream_forward()
        torch.add(depth, prior, out=out)
        if masked:
            mask.sum()

    pixels = H * W
    fwd = _alternate({"torch": lambda: forward(composed), "fused": lambda: forward(fused), "stream": stream_forward},
                     args)
    both = _alternate({"torch": lambda: forward_backward(composed), "fused": lambda: forward_backward(fused),
                       "stream": stream_both}, args)
    return dict(height=H, width=W, pixels=pixels, masked=bool(masked), loss=loss,
                forward=_summarise(fwd, forward_bytes(pixels, masked, loss)),
                forward_backward=_summarise(both, forward_bytes(pixels, masked, loss) + backward_bytes(pixels, masked)))


def bench_training(args, shape):
    """one training iteration with no depth loss, the HIP operator or the torch composition added to the photometric loss"""
    H, W = shape
    dev = args.device
    g, camera = scenes.benchmark_scene(args.n, (W, H), sh_degree=3, seed=args.seed)
    cam, cfg = camera.to(device=dev), RasterConfig()
    gen = torch.Generator().manual_seed(args.seed + 1)
    target = torch.rand(H, W, 3, generator=gen).to(dev)
    g = g.to(dev)
    with torch.no_grad():
        first = render_gaussians(g, cam, cfg, use_sh=True, render_depth=True)
        prior = 2.0 / first.depth.clamp_min(1e-3) + 0.1 + 0.01 * torch.randn(H, W, generator=gen).to(dev)

    def iteration(fn):
        gd = g.detach().requires_grad_(True)
        r = render_gaussians(gd, cam, cfg, use_sh=True, render_depth=True)
        loss = losses.photometric_loss(r.image, target)
        if fn is not None:
            loss = loss + 0.1 * fn(r.depth, prior, r.image_weight.detach() > 0.5)
        loss.backward()

    paths = _alternate({"alone": lambda: iteration(None), "torch": lambda: iteration(torch_depth_prior_loss),
                        "fused": lambda: iteration(fused_affine)}, args)
    fused, composed, alone = paths["fused"], paths["torch"], paths["alone"]
    paths.update(height=H, width=W, n=args.n, added_ms=fused["ms"] - alone["ms"],
                 added_torch_ms=composed["ms"] - alone["ms"],
                 fused_faster=composed["ms"] - fused["ms"] > max(composed["spread_ms"], fused["spread_ms"]))
    return paths


def bench_depth_loss(args):
    sizes, train_shape = SIZES, (1080, 1920)
    if args.depth_size:
        h, w = (int(v) for v in args.depth_size.split(","))
        sizes, train_shape = ((h, w),), (h, w)
    record = dict(warmup=args.warmup, iters=args.iters, rounds=args.rounds,
                  cases=[bench_case(args, shape, masked, loss) for shape in sizes for masked in (False, True)
                         for loss in LOSSES],
                  training=bench_training(args, train_shape))
    for case in record["cases"]:
        print(f"{case['height']} x {case['width']}, {case['loss']}, {'masked' if case['masked'] else 'no mask'}")
        for part in ("forward", "forward_backward"):
            r = case[part]
            print(f"  {part}: fused {r['fused']['ms']:.4f} ms (spread {r['fused']['spread_ms']:.4f}), torch "
                  f"{r['torch']['ms']:.4f} ms (spread {r['torch']['spread_ms']:.4f}), stream {r['stream']['ms']:.4f} ms "
                  f"(spread {r['stream']['spread_ms']:.4f}); {r['bytes']} bytes: fused {r['fused_tbps']:.2f} TB/s, "
                  f"stream {r['stream_tbps']:.2f} TB/s, fused / stream {r['ratio_to_stream']:.2f}, torch / fused "
                  f"{r['speedup']:.1f}; fused faster by more than the spread: {r['fused_faster']}")
    t = record["training"]
    print(f"training iteration, {t['n']} Gaussians at {t['height']} x {t['width']} with render_depth: alone "
          f"{t['alone']['ms']:.3f} ms (spread {t['alone']['spread_ms']:.3f}), with depth_prior_loss "
          f"{t['fused']['ms']:.3f} ms (spread {t['fused']['spread_ms']:.3f}, + {t['added_ms']:.3f}), with the torch "
          f"composition {t['torch']['ms']:.3f} ms (spread {t['torch']['spread_ms']:.3f}, + {t['added_torch_ms']:.3f}); "
          f"fused faster by more than the spread: {t['fused_faster']}")
    return record


def main():
    args = parse_args()
    record = bench_depth_loss(args)
    print(json.dumps(record))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)
    return record


if __name__ == "__main__":
    main()
