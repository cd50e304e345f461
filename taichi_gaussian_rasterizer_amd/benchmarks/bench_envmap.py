"""environment.composite_environment against the same operation composed in torch, and against plain streaming.

Shapes: 2048 x 2048 x 3 and 1080 x 1920 x 3 under the benchmark scene's camera, over maps of edge 64, 512 and 2048 --
the map's gradient runs its group kernel (four waves per texel), its lane kernel at a few pixels per texel and its lane
kernel below one pixel per texel -- with three image weights: `horizon` (sky above a soft horizon, full coverage
below), `sky` (weight 0 everywhere) and `noise`.  `--envmap_size H,W` runs that one size over edges 64 and 512
instead.  Per shape, forward (no autograd graph) and forward + backward (gradients for the map and the weight, as in
training) of
  fused   composite_environment
  torch   the formula with index gathers (the map's gradient is an index_put with float atomics)
  stream  passes that move the bytes the operation cannot avoid: forward reads the image and the weight and writes the
          image (4 (2 C + 1) bytes per pixel), backward also reads the incoming gradient (4 C per pixel) and writes
          the map's gradient (24 R^2 C)
all on the device, the three alternating round by round: `--warmup` calls, then `--iters` calls between two events;
`--rounds` rounds, median of the rounds, spread = largest minus smallest round.  fused_faster: the torch composition is
slower by more than either spread.  One more row: a training iteration (render_gaussians(differentiable_weight=True) +
photometric loss + backward, `--n` Gaussians at 1920 x 1080, or at the one size) alone, with composite_environment over
an edge of 512 in front of the loss, and with the torch composition there.
--json PATH writes the record."""
from __future__ import annotations

import json

import torch

from .. import losses, scenes
from ..data_types import RasterConfig
from ..environment import composite_environment
from ..renderer import render_gaussians
from .bench_bilagrid import _alternate, _summarise
from .util import FLAGS, make_parser

FLAGS.setdefault("rounds", dict(type=int, default=3))
FLAGS.setdefault("warmup", dict(type=int, default=3))
FLAGS.setdefault("envmap_size", dict(type=str, default="", help="H,W: run this one size instead of the standard shapes"))
parse_args = make_parser(("device", "seed", "iters", "json", "rounds", "warmup", "envmap_size", "n"), iters=20, n=200000)

SIZES = ((2048, 2048), (1080, 1920))
EDGES = (64, 512, 2048)
WEIGHTS = ("horizon", "sky", "noise")
CHANNELS = 3
TRAIN_EDGE = 512
_OTHERS = ((1, 2), (0, 2), (0, 1))


def forward_bytes(pixels, channels=CHANNELS):
    return 4 * (2 * channels + 1) * pixels


def backward_bytes(pixels, edge, channels=CHANNELS):
    return 4 * channels * pixels + 24 * edge * edge * channels


def torch_composite(env, image, weight, camera):
    """the module's formula as a trainer composes it today: a direction per pixel, a face select, four gathers"""
    R = env.shape[1]
    W, H = camera.image_size
    proj, T = camera.projection, camera.T_camera_world
    x = torch.arange(W, dtype=proj.dtype, device=proj.device)
    y = torch.arange(H, dtype=proj.dtype, device=proj.device)
    dx = ((x + 0.5 - proj[2]) / proj[0]).view(1, W).expand(H, W)
    dy = ((y + 0.5 - proj[3]) / proj[1]).view(H, 1).expand(H, W)
    d = torch.stack([dx, dy, torch.ones_like(dx)], dim=-1) @ T[:3, :3]
    axis = d.abs().argmax(dim=-1)
    d_a = d.gather(-1, axis[..., None])[..., 0]
    face = 2 * axis + (d_a < 0).long()
    first = torch.tensor([o[0] for o in _OTHERS], device=d.device)[axis]
    second = torch.tensor([o[1] for o in _OTHERS], device=d.device)[axis]
    u = ((d.gather(-1, first[..., None])[..., 0] / d_a.abs() + 1) / 2 * R - 0.5).clamp(0, R - 1)
    v = ((d.gather(-1, second[..., None])[..., 0] / d_a.abs() + 1) / 2 * R - 0.5).clamp(0, R - 1)
    i0, j0 = u.floor().long().clamp(max=R - 1), v.floor().long().clamp(max=R - 1)
    i1, j1 = (i0 + 1).clamp(max=R - 1), (j0 + 1).clamp(max=R - 1)
    fu, fv = (u - i0)[..., None], (v - j0)[..., None]
    top = env[face, j0, i0] + (env[face, j0, i1] - env[face, j0, i0]) * fu
    bot = env[face, j1, i0] + (env[face, j1, i1] - env[face, j1, i0]) * fu
    sky = top + (bot - top) * fv
    return sky if image is None else image + (1 - weight)[..., None] * sky


def make_weight(kind, H, W, gen):
    if kind == "sky":
        return torch.zeros(H, W)
    if kind == "noise":
        return torch.rand(H, W, generator=gen)
    rows = (torch.arange(H) + 0.5) / H  # a horizon at mid height, 5 % of the height soft
    return ((rows - 0.5) / 0.05).clamp(0, 1).view(H, 1).expand(H, W).contiguous()


def bench_case(args, shape, edge, kind):
    H, W = shape
    dev = args.device
    gen = torch.Generator().manual_seed(args.seed)
    cam = scenes.benchmark_camera((W, H)).to(device=dev)
    image = torch.rand(H, W, CHANNELS, generator=gen).to(dev)
    weight = make_weight(kind, H, W, gen).to(dev)
    upstream = (torch.rand(H, W, CHANNELS, generator=gen) - 0.5).to(dev)
    env = torch.rand(6, edge, edge, CHANNELS, generator=gen).to(dev)
    out, d_env = torch.empty_like(image), torch.empty_like(env)

    def forward(fn):
        with torch.no_grad():
            fn(env, image, weight, cam)

    def forward_backward(fn):
        e, w = env.detach().requires_grad_(True), weight.detach().requires_grad_(True)
        fn(e, image, w, cam).backward(upstream)

    def stream_forward():
        torch.add(image, weight.unsqueeze(-1), out=out)

    def stream_both():
        torch.add(image, weight.unsqueeze(-1), out=out)
        upstream.sum()
        d_env.fill_(0.0)

    pixels = H * W
    fwd = _alternate({"torch": lambda: forward(torch_composite), "fused": lambda: forward(composite_environment),
                      "stream": stream_forward}, args)
    both = _alternate({"torch": lambda: forward_backward(torch_composite),
                       "fused": lambda: forward_backward(composite_environment), "stream": stream_both}, args)
    return dict(height=H, width=W, edge=edge, channels=CHANNELS, weight=kind, pixels=pixels,
                forward=_summarise(fwd, forward_bytes(pixels)),
                forward_backward=_summarise(both, forward_bytes(pixels) + backward_bytes(pixels, edge)))


def bench_training(args, shape):
    """one training iteration with nothing, the HIP operator or the torch composition between render and loss"""
    H, W = shape
    dev = args.device
    g, camera = scenes.benchmark_scene(args.n, (W, H), sh_degree=3, seed=args.seed)
    cam, cfg = camera.to(device=dev), RasterConfig()
    gen = torch.Generator().manual_seed(args.seed + 1)
    target = torch.rand(H, W, 3, generator=gen).to(dev)
    env0 = torch.rand(6, TRAIN_EDGE, TRAIN_EDGE, 3, generator=gen).to(dev)
    g = g.to(dev)

    def iteration(fn):
        gd = g.detach().requires_grad_(True)
        r = render_gaussians(gd, cam, cfg, use_sh=True, differentiable_weight=True)
        image = r.image
        if fn is not None:
            image = fn(env0.detach().requires_grad_(True), r.image, r.image_weight, cam)
        losses.photometric_loss(image, target).backward()

    paths = _alternate({"alone": lambda: iteration(None), "torch": lambda: iteration(torch_composite),
                        "fused": lambda: iteration(composite_environment)}, args)
    fused, composed, alone = paths["fused"], paths["torch"], paths["alone"]
    paths.update(height=H, width=W, n=args.n, edge=TRAIN_EDGE, added_ms=fused["ms"] - alone["ms"],
                 added_torch_ms=composed["ms"] - alone["ms"],
                 fused_faster=composed["ms"] - fused["ms"] > max(composed["spread_ms"], fused["spread_ms"]))
    return paths


def bench_envmap(args):
    sizes, edges, train_shape = SIZES, EDGES, (1080, 1920)
    if args.envmap_size:
        h, w = (int(v) for v in args.envmap_size.split(","))
        sizes, edges, train_shape = ((h, w),), EDGES[:2], (h, w)
    record = dict(warmup=args.warmup, iters=args.iters, rounds=args.rounds,
                  cases=[bench_case(args, shape, edge, kind) for shape in sizes for edge in edges for kind in WEIGHTS],
                  training=bench_training(args, train_shape))
    for case in record["cases"]:
        print(f"{case['height']} x {case['width']} x {case['channels']}, weight {case['weight']}, over a map of edge "
              f"{case['edge']}")
        for part in ("forward", "forward_backward"):
            r = case[part]
            print(f"  {part}: fused {r['fused']['ms']:.4f} ms (spread {r['fused']['spread_ms']:.4f}), torch "
                  f"{r['torch']['ms']:.4f} ms (spread {r['torch']['spread_ms']:.4f}), stream {r['stream']['ms']:.4f} ms "
                  f"(spread {r['stream']['spread_ms']:.4f}); {r['bytes']} bytes: fused {r['fused_tbps']:.2f} TB/s, "
                  f"stream {r['stream_tbps']:.2f} TB/s, fused / stream {r['ratio_to_stream']:.2f}, torch / fused "
                  f"{r['speedup']:.1f}; fused faster by more than the spread: {r['fused_faster']}")
    t = record["training"]
    print(f"training iteration, {t['n']} Gaussians at {t['height']} x {t['width']}, map of edge {t['edge']}: alone "
          f"{t['alone']['ms']:.3f} ms (spread {t['alone']['spread_ms']:.3f}), with composite_environment "
          f"{t['fused']['ms']:.3f} ms (spread {t['fused']['spread_ms']:.3f}, + {t['added_ms']:.3f}), with the torch "
          f"composition {t['torch']['ms']:.3f} ms (spread {t['torch']['spread_ms']:.3f}, + {t['added_torch_ms']:.3f}); "
          f"fused faster by more than the spread: {t['fused_faster']}")
    return record


def main():
    args = parse_args()
    record = bench_envmap(args)
    print(json.dumps(record))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)
    return record


if __name__ == "__main__":
    main()
