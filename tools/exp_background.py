"""Background colour and differentiable image_weight: what the in-kernel route costs, on bench.py's c3 frame
(1 M Gaussians, 2048 x 2048, forward + backward from fixed random upstream gradients).
  A  SH degree 3 (the benchmark's own configuration): the default frame against the frame with `background` and
     `differentiable_weight` on (loss on image and image_weight).
  B  plain features, C = 3, the same Gaussians: the default frame, the in-kernel route, and the same effect composed in
     torch on the old path -- a constant-1 fourth feature channel (its blend IS the weight, with a gradient) and
     image[..., :3] + (1 - image[..., 3:]) * background.
  One elementwise pass over the (H, W, 3) image (torch.add of a scalar) is timed as the yardstick.
The variants are interleaved, --rounds times, --iters synchronised frames each after --warmup; per variant the median
of each round, so that the spread between rounds of one variant is visible next to the differences between variants.
Usage: python tools/exp_background.py [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import taichi_gaussian_rasterizer_amd as gs  # noqa: E402
from taichi_gaussian_rasterizer_amd import RasterConfig, scenes  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--n", type=int, default=1_000_000)
p.add_argument("--image_size", type=str, default="2048,2048")
p.add_argument("--rounds", type=int, default=3)
p.add_argument("--warmup", type=int, default=5)
p.add_argument("--iters", type=int, default=20)
p.add_argument("--out", type=str, default=None)
args = p.parse_args()
size = tuple(int(x) for x in args.image_size.split(","))
W, H = size
dev = "cuda:0"
cfg = RasterConfig()

g_cpu, cam_cpu = scenes.benchmark_scene(args.n, size, sh_degree=3, seed=0)
cam = cam_cpu.to(device=dev)
gen = torch.Generator().manual_seed(1)
G = torch.rand(H, W, 3, generator=gen).to(dev)
GW = (torch.rand(H, W, generator=gen) * 2 - 1).to(dev)
bg = torch.rand(3, generator=gen).to(dev)
sh = g_cpu.to(dev).requires_grad_(True)
colours = torch.rand(args.n, 3, generator=gen)
plain = g_cpu.replace(feature=colours).to(dev).requires_grad_(True)
ones = g_cpu.replace(feature=torch.cat((colours, torch.ones(args.n, 1)), 1)).to(dev).requires_grad_(True)


def clear(g):
    for _, t in g.items():
        t.grad = None


def frame(g, use_sh, new):
    clear(g)
    if new:
        r = gs.render_gaussians(g, cam, cfg, use_sh=use_sh, background=bg, differentiable_weight=True)
        torch.autograd.backward([r.image, r.image_weight], [G, GW])
    else:
        r = gs.render_gaussians(g, cam, cfg, use_sh=use_sh)
        r.image.backward(G)


def torch_composite():
    clear(ones)
    r = gs.render_gaussians(ones, cam, cfg)
    weight = r.image[..., 3]
    image = r.image[..., :3] + (1 - weight).unsqueeze(-1) * bg
    torch.autograd.backward([image, weight], [G, GW])


image = torch.rand(H, W, 3, device=dev)
VARIANTS = {
    "A_sh3_default": lambda: frame(sh, True, False),
    "A_sh3_background_weight": lambda: frame(sh, True, True),
    "B_plain_default": lambda: frame(plain, False, False),
    "B_plain_background_weight": lambda: frame(plain, False, True),
    "B_plain_ones_channel_torch_composite": torch_composite,
    "elementwise_pass_over_image": lambda: torch.add(image, 1.0),
}


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


rounds = {name: [] for name in VARIANTS}
for _ in range(args.rounds):
    for name, fn in VARIANTS.items():
        rounds[name].append(round(timed(fn), 4))
        print(name, rounds[name][-1], flush=True)


def mid(name):
    return sorted(rounds[name])[len(rounds[name]) // 2]


result = dict(device=torch.cuda.get_device_name(0), n=args.n, image_size=list(size), rounds=args.rounds,
              iters=args.iters, warmup=args.warmup, ms_per_frame_median_of_each_round=rounds,
              ms_per_frame={name: mid(name) for name in VARIANTS},
              spread_ms={name: round(max(v) - min(v), 4) for name, v in rounds.items()},
              A_in_kernel_extra_ms=round(mid("A_sh3_background_weight") - mid("A_sh3_default"), 4),
              B_in_kernel_extra_ms=round(mid("B_plain_background_weight") - mid("B_plain_default"), 4),
              B_torch_route_extra_ms=round(mid("B_plain_ones_channel_torch_composite") - mid("B_plain_default"), 4))
text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
