"""Wide features: rasterizer forward / backward time at F = 32, 64, 128, 256 on the operator benchmark's scene
(benchmarks/bench_rasterizer.py defaults: 1 M splats, 1024 x 768, tile 16, scale_factor 4), three ways:
  wide    gs_raster_fwd_wide / gs_raster_bwd_wide on all F channels
  sliced  ceil(F / 32) calls of gs_raster_fwd / gs_raster_bwd on 32-channel slices (the caller-side workaround)
  narrow  gs_raster_fwd / gs_raster_bwd at F = 32 (one slice)
Each time includes the zero-fills the Python layer does (and the narrow backward's row unpack); slices are cut
before timing.  Median of --iters timed calls after --warmup.  Usage: python tools/exp_wide_features.py [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from taichi_gaussian_rasterizer_amd import RasterConfig, _native as nv  # noqa: E402
from taichi_gaussian_rasterizer_amd.mapper.tile_mapper import map_to_tiles  # noqa: E402
from taichi_gaussian_rasterizer_amd.misc.renderer2d import project_gaussians2d  # noqa: E402
from taichi_gaussian_rasterizer_amd.scenes import random_2d_gaussians  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--n", type=int, default=1_000_000)
p.add_argument("--image_size", type=str, default="1024,768")
p.add_argument("--widths", type=str, default="32,64,128,256")
p.add_argument("--warmup", type=int, default=3)
p.add_argument("--iters", type=int, default=10)
p.add_argument("--out", type=str, default=None)
args = p.parse_args()
size = tuple(int(x) for x in args.image_size.split(","))
widths = [int(x) for x in args.widths.split(",")]
w, h = size
dev = "cuda:0"
lib = nv.lib()

torch.manual_seed(0)
scene = random_2d_gaussians(args.n, size, num_channels=max(widths), scale_factor=4, alpha_range=(0.75, 1.0),
                            depth_range=(0.1, 100.0)).to(dev)
cfg = RasterConfig()
splats = project_gaussians2d(scene).contiguous()
o2p, ranges = map_to_tiles(splats, depth=scene.z_depth, image_size=size, config=cfg)
ranges = ranges.view(-1, 2).contiguous()
c = nv.make_config(cfg)
v, k = splats.shape[0], o2p.shape[0]
lines = [f"scene: {args.n} splats, {w}x{h}, tile 16, K = {k} overlaps ({k / ranges.shape[0]:.0f} per tile)"]


def timed(fn):
    for _ in range(args.warmup):
        fn()
    ts = []
    for _ in range(args.iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def narrow_fwd(f, image, alpha):
    nv.check(lib.gs_raster_fwd(v, f.shape[1], nv.ptr(splats), nv.ptr(f), nv.ptr(ranges), nv.ptr(o2p), k, w, h, c, None,
                               None, nv.ptr(image), nv.ptr(alpha), None, None, None, 0, nv.stream()), "gs_raster_fwd")


def narrow_bwd(f, image, gi):
    F = f.shape[1]
    rows = torch.zeros((v, lib.gs_grad_row_floats(F)), device=dev)
    nv.check(lib.gs_raster_bwd(v, F, nv.ptr(splats), nv.ptr(f), nv.ptr(ranges), nv.ptr(o2p), k, w, h, c, None, None,
                               nv.ptr(image), nv.ptr(gi), None, None, nv.ptr(rows), None, nv.stream()), "gs_raster_bwd")
    gg, gf = torch.empty((v, 7), device=dev), torch.empty((v, F), device=dev)
    nv.check(lib.gs_raster_bwd_unpack(v, F, nv.ptr(rows), nv.ptr(gg), nv.ptr(gf), None, nv.stream()), "unpack")


def wide_fwd(f, image, alpha):
    nv.check(lib.gs_raster_fwd_wide(v, f.shape[1], nv.ptr(splats), nv.ptr(f), nv.ptr(ranges), nv.ptr(o2p), k, w, h, c,
                                    nv.ptr(image), nv.ptr(alpha), None, None, 0, nv.stream()), "gs_raster_fwd_wide")


def wide_bwd(f, image, gi):
    F = f.shape[1]
    gg, gf = torch.zeros((v, 7), device=dev), torch.zeros((v, F), device=dev)
    nv.check(lib.gs_raster_bwd_wide(v, F, nv.ptr(splats), nv.ptr(f), nv.ptr(ranges), nv.ptr(o2p), k, w, h, c,
                                    nv.ptr(image), nv.ptr(gi), None, None, nv.ptr(gg), nv.ptr(gf), None, nv.stream()),
             "gs_raster_bwd_wide")


results = []
for F in widths:
    f = scene.feature[:, :F].contiguous()
    image, alpha = torch.empty((h, w, F), device=dev), torch.empty((h, w), device=dev)
    gi = torch.rand((h, w, F), device=dev, generator=torch.Generator(device=dev).manual_seed(F))
    wide_fwd(f, image, alpha)
    slices = [(f[:, c0:c0 + 32].contiguous(), image[..., c0:c0 + 32].contiguous(), gi[..., c0:c0 + 32].contiguous())
              for c0 in range(0, F, 32)]
    s_img, s_alpha = torch.empty((h, w, 32), device=dev), torch.empty((h, w), device=dev)
    r = dict(F=F,
             wide_fwd_ms=timed(lambda: wide_fwd(f, image, alpha)),
             wide_bwd_ms=timed(lambda: wide_bwd(f, image, gi)),
             sliced_fwd_ms=timed(lambda: [narrow_fwd(sf, s_img, s_alpha) for sf, _, _ in slices]),
             sliced_bwd_ms=timed(lambda: [narrow_bwd(sf, si, sg) for sf, si, sg in slices]))
    if F == 32:
        r["narrow_fwd_ms"], r["narrow_bwd_ms"] = r.pop("sliced_fwd_ms"), r.pop("sliced_bwd_ms")
    r = {key: (round(val, 4) if isinstance(val, float) else val) for key, val in r.items()}
    results.append(r)
    lines.append(json.dumps(r))
    print(lines[-1], flush=True)
    del f, image, alpha, gi, slices

lines.insert(1, f"device: {torch.cuda.get_device_name(0)}; median of {args.iters} calls after {args.warmup} warm-up")
text = "\n".join(lines) + "\n"
print(lines[0])
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
