"""appearance.slice_bilateral_grid against the same operation composed in torch, and against plain streaming.

Shapes: 2048 x 2048 x 3 and 1080 x 1920 x 3 under an (8, 16, 16) grid, 2048 x 2048 x 3 under a (1, 1, 1) grid (the
per-image colour matrix); `--bilagrid_size H,W` runs that one size under both grids instead.  The image is uniform noise
in [0, 1]: every wave meets every level of the grid, the most work the backward's per-cell reduction can get.  The first
shape runs once more on a smooth image (low-frequency waves, as the sky, walls and gradients of a photo), where a wave
meets one or two cells.  Per shape, forward (no autograd graph) and forward + backward (gradients for the grid and the
image, as in training) of
  fused   slice_bilateral_grid
  torch   grid_sample(bilinear, border, align_corners) on a (1, 1, H, W, 3) coordinate tensor + the affine as a matmul
  stream  torch.add passes that move the bytes the operation cannot avoid: forward reads and writes one image (24 bytes
          per pixel), backward reads the image and the incoming gradient and writes d_image (36 bytes per pixel)
all on the device, the three alternating round by round: `--warmup` calls, then `--iters` calls between two events;
`--rounds` rounds, median of the rounds, spread = largest minus smallest round.  bytes / ms gives the TB/s of the fused
and the streaming path; fused_faster: the torch composition is slower by more than either spread.  At these sizes the
images stay in the 256 MiB last-level cache from call to call, for all three paths alike.
--json PATH writes the record."""
from __future__ import annotations

import json
import statistics

import torch
import torch.nn.functional as F

from ..appearance import identity_grids, slice_bilateral_grid
from .util import FLAGS, make_parser

FLAGS.setdefault("rounds", dict(type=int, default=3))
FLAGS.setdefault("warmup", dict(type=int, default=3))
FLAGS.setdefault("bilagrid_size", dict(type=str, default="", help="H,W: run this one size instead of the standard shapes"))
parse_args = make_parser(("device", "seed", "iters", "json", "rounds", "warmup", "bilagrid_size"), iters=20)

CASES = (((2048, 2048), (8, 16, 16), "noise"), ((1080, 1920), (8, 16, 16), "noise"), ((2048, 2048), (1, 1, 1), "noise"),
         ((2048, 2048), (8, 16, 16), "smooth"))
FORWARD_BYTES, BACKWARD_BYTES = 24, 36  # per pixel
LUMA = (0.299, 0.587, 0.114)


def torch_slice(grid, image):
    """the composition a trainer writes today: grid (12, L, Hg, Wg), image (H, W, 3)"""
    H, W, _ = image.shape
    u = ((torch.arange(W, dtype=image.dtype, device=image.device) + 0.5) / W).expand(H, W)
    v = ((torch.arange(H, dtype=image.dtype, device=image.device) + 0.5) / H).view(H, 1).expand(H, W)
    luma = (image * image.new_tensor(LUMA)).sum(-1)
    coords = torch.stack([u, v, luma], dim=-1) * 2 - 1
    A = F.grid_sample(grid[None], coords[None, None], mode="bilinear", padding_mode="border", align_corners=True)
    A = A[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
    return (A[..., :3] @ image[..., None])[..., 0] + A[..., 3]


def _event_ms(f, iters):
    first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    first.record()
    for _ in range(iters):
        f()
    last.record()
    torch.cuda.synchronize()
    return first.elapsed_time(last) / iters


def _alternate(paths, args):
    rounds = {name: [] for name in paths}
    for _ in range(args.rounds):
        for name, f in paths.items():
            for _ in range(args.warmup):
                f()
            torch.cuda.synchronize()
            rounds[name].append(_event_ms(f, args.iters))
    return {name: dict(rounds=r, ms=statistics.median(r), spread_ms=max(r) - min(r)) for name, r in rounds.items()}


def _summarise(record, nbytes):
    fused, composed, stream = record["fused"], record["torch"], record["stream"]
    record.update(bytes=nbytes, fused_tbps=nbytes / (fused["ms"] * 1e-3) / 1e12,
                  stream_tbps=nbytes / (stream["ms"] * 1e-3) / 1e12, ratio_to_stream=fused["ms"] / stream["ms"],
                  speedup=composed["ms"] / fused["ms"],
                  fused_faster=composed["ms"] - fused["ms"] > max(composed["spread_ms"], fused["spread_ms"]))
    return record


def smooth_image(H, W):
    """three low-frequency waves in [0.1, 0.9], one per channel"""
    u = ((torch.arange(W) + 0.5) / W).view(1, W, 1)
    v = ((torch.arange(H) + 0.5) / H).view(H, 1, 1)
    phase = torch.tensor([0.0, 0.9, 2.1]).view(1, 1, 3)
    return 0.5 + 0.4 * torch.sin(6.283185 * (1.5 * u + 0.7 * v) + phase) * torch.cos(6.283185 * (0.8 * v - 0.3 * u))


def bench_case(args, shape, sizes, kind="noise"):
    H, W = shape
    dev = args.device
    gen = torch.Generator().manual_seed(args.seed)
    image = (torch.rand(H, W, 3, generator=gen) if kind == "noise" else smooth_image(H, W)).to(dev)
    upstream = (torch.rand(H, W, 3, generator=gen) - 0.5).to(dev)
    grid = (identity_grids(1, *sizes)[0] + 0.1 * (torch.rand(12, *sizes, generator=gen) - 0.5)).to(dev)
    out, d_image = torch.empty_like(image), torch.empty_like(image)

    def forward(fn):
        with torch.no_grad():
            fn(grid, image)

    def forward_backward(fn):
        g, x = grid.detach().requires_grad_(True), image.detach().requires_grad_(True)
        fn(g, x).backward(upstream)

    def stream_forward():
        torch.add(image, 1.0, out=out)

    def stream_both():
        torch.add(image, 1.0, out=out)
        torch.add(image, upstream, out=d_image)

    pixels = H * W
    fwd = _alternate({"torch": lambda: forward(torch_slice), "fused": lambda: forward(slice_bilateral_grid),
                      "stream": stream_forward}, args)
    both = _alternate({"torch": lambda: forward_backward(torch_slice),
                       "fused": lambda: forward_backward(slice_bilateral_grid), "stream": stream_both}, args)
    return dict(height=H, width=W, grid=list(sizes), image=kind, pixels=pixels,
                forward=_summarise(fwd, FORWARD_BYTES * pixels),
                forward_backward=_summarise(both, (FORWARD_BYTES + BACKWARD_BYTES) * pixels))


def bench_bilagrid(args):
    cases = CASES
    if args.bilagrid_size:
        h, w = (int(v) for v in args.bilagrid_size.split(","))
        cases = (((h, w), (8, 16, 16), "noise"), ((h, w), (1, 1, 1), "noise"))
    record = dict(warmup=args.warmup, iters=args.iters, rounds=args.rounds,
                  cases=[bench_case(args, shape, sizes, kind) for shape, sizes, kind in cases])
    for case in record["cases"]:
        print(f"{case['height']} x {case['width']} x 3 ({case['image']}) under a grid {tuple(case['grid'])}")
        for part in ("forward", "forward_backward"):
            r = case[part]
            print(f"  {part}: fused {r['fused']['ms']:.4f} ms (spread {r['fused']['spread_ms']:.4f}), torch "
                  f"{r['torch']['ms']:.4f} ms (spread {r['torch']['spread_ms']:.4f}), stream {r['stream']['ms']:.4f} ms "
                  f"(spread {r['stream']['spread_ms']:.4f}); {r['bytes']} bytes: fused {r['fused_tbps']:.2f} TB/s, "
                  f"stream {r['stream_tbps']:.2f} TB/s, fused / stream {r['ratio_to_stream']:.2f}, torch / fused "
                  f"{r['speedup']:.1f}; fused faster by more than the spread: {r['fused_faster']}")
    return record


def main():
    args = parse_args()
    record = bench_bilagrid(args)
    print(json.dumps(record))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)
    return record


if __name__ == "__main__":
    main()
