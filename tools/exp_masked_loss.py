"""Time the photometric loss of whichever package PYTHONPATH gives, forward+backward at 2048x2048x3 and 1920x1080x3:
the unmasked fused loss, the masked fused loss (if that package has mask=), and the same masked numbers from the
operators without mask= (the SSIM map weighted by torch ops and a torch L1).  Device events around every call,
alternated rounds, medians; also hashes of the results, to compare two builds bit for bit.

A/B against another commit in one session, separate processes, in the order other / this / other
(profiles/masked_loss/): check that commit out into a directory of its own, build it, and run

    PYTHONPATH=<that tree> python tools/exp_masked_loss.py --label parent1 --out parent1.json
    PYTHONPATH=.           python tools/exp_masked_loss.py --label new     --out new.json
    PYTHONPATH=<that tree> python tools/exp_masked_loss.py --label parent2 --out parent2.json
"""
import argparse
import hashlib
import inspect
import json
import statistics

import torch

import taichi_gaussian_rasterizer_amd as pkg
from taichi_gaussian_rasterizer_amd.losses import photometric_loss, ssim

p = argparse.ArgumentParser()
p.add_argument("--label", required=True)
p.add_argument("--out", required=True)
p.add_argument("--warmup", type=int, default=20)
p.add_argument("--iters", type=int, default=200)
p.add_argument("--rounds", type=int, default=3)
args = p.parse_args()
DEV = "cuda:0"
HAS_MASK = "mask" in inspect.signature(photometric_loss).parameters


def map_masked_loss(image, target, mask, ssim_weight=0.2):
    w = mask.unsqueeze(-1)
    norm = image.shape[-1] * mask.sum()
    ssim_mean = (ssim(image, target, reduction="none") * w).sum() / norm
    l1 = ((image - target).abs() * w).sum() / norm
    return (1 - ssim_weight) * l1 + ssim_weight * (1 - ssim_mean)


def call_times(f, iters):
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in events:
        a.record()
        f()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in events]


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


record = dict(label=args.label, package=pkg.__file__, has_mask=HAS_MASK, warmup=args.warmup, iters=args.iters,
              rounds=args.rounds, sizes={})
for w, h in ((2048, 2048), (1920, 1080)):
    gen = torch.Generator().manual_seed(0)
    target = torch.rand(h, w, 3, generator=gen)
    image = (target + 0.05 * (torch.rand(h, w, 3, generator=gen) - 0.5)).to(DEV).requires_grad_(True)
    target = target.to(DEV)
    mask = torch.rand(h, w, generator=gen).to(DEV)
    out = {}

    def fused():
        image.grad = None
        loss = photometric_loss(image, target)
        loss.backward()
        return loss

    def fused_masked():
        image.grad = None
        loss = photometric_loss(image, target, mask=mask)
        loss.backward()
        return loss

    def map_masked():
        image.grad = None
        loss = map_masked_loss(image, target, mask)
        loss.backward()
        return loss

    steps = {"fused forward+backward": fused, "map + torch masked forward+backward": map_masked}
    if HAS_MASK:
        steps["fused masked forward+backward"] = fused_masked
    medians = {k: [] for k in steps}
    for _ in range(args.rounds):
        for name, f in steps.items():
            for _ in range(args.warmup):
                f()
            torch.cuda.synchronize()
            medians[name].append(statistics.median(call_times(f, args.iters)))
    for name, f in steps.items():
        loss = f()
        torch.cuda.synchronize()
        out[name] = dict(ms_rounds=medians[name], ms=statistics.median(medians[name]),
                         spread_ms=max(medians[name]) - min(medians[name]), loss=float(loss),
                         loss_bits=digest(loss), d_image_bits=digest(image.grad))
    if HAS_MASK:
        a, b = out["fused masked forward+backward"], out["map + torch masked forward+backward"]
        map_masked()
        g_map = image.grad.clone()
        fused_masked()
        out["masked_vs_map_max_abs_grad_diff"] = float((image.grad - g_map).abs().max())
        out["masked_vs_map_max_abs_grad"] = float(g_map.abs().max())
        out["masked_vs_map_loss_diff"] = abs(a["loss"] - b["loss"])
    record["sizes"][f"{w}x{h}x3"] = out
    for name, v in out.items():
        print(args.label, f"{w}x{h}", name, v if not isinstance(v, dict) else (v["ms"], v["ms_rounds"], v["loss"]))
with open(args.out, "w") as fh:
    json.dump(record, fh, indent=1)
