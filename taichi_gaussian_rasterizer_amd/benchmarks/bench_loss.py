"""Photometric loss (1 - w) * L1 + w * (1 - SSIM): the fused HIP kernels against the same loss composed from torch ops
(grouped conv2d on channel-first copies, as a trainer without this package writes it).

Phases: fused forward (no_grad), fused forward+backward, torch forward+backward, l1 only (fused, ssim_weight = 0),
fused masked forward+backward (mask= with U(0, 1) weights), map + torch masked forward+backward (the same numbers
without mask=: the SSIM map weighted by torch ops and a torch L1).
For the fused phases the compulsory traffic, 44 bytes per pixel-channel forward+backward (8 forward only), over the
time is printed as a share of the 6.29 TB/s copy rate.  --json PATH: additionally time fused and torch
forward+backward call by call, alternating, twice each, and write the medians and their spread."""
from __future__ import annotations

import json
import statistics

import torch
import torch.nn.functional as F

from ..losses import photometric_loss, ssim
from .util import Phases, make_parser

parse_args = make_parser(("profile", "image_size", "device", "seed", "iters", "num_channels", "ssim_weight", "json",
                          "debug"), image_size="2048,2048", iters=100)

COPY_RATE = 6.29e12  # bytes / s, float4 copy on the MI355X
BYTES_FWD_BWD, BYTES_FWD = 44, 8


def torch_window(channels, device, window_size=11, sigma=1.5):
    x = torch.arange(window_size, dtype=torch.float64) - (window_size - 1) / 2
    g = torch.exp(-x * x / (2 * sigma * sigma))
    g = (g / g.sum()).float()
    return torch.outer(g, g).expand(channels, 1, window_size, window_size).contiguous().to(device)


def torch_photometric_loss(image, target, window, ssim_weight=0.2):
    """the composition a caller writes today: channel-last in, permuted to channel-first for conv2d"""
    x = image.permute(2, 0, 1).unsqueeze(0).contiguous()
    y = target.permute(2, 0, 1).unsqueeze(0).contiguous()
    C, pad = x.shape[1], window.shape[-1] // 2
    mu_x, mu_y = F.conv2d(x, window, padding=pad, groups=C), F.conv2d(y, window, padding=pad, groups=C)
    var_x = F.conv2d(x * x, window, padding=pad, groups=C) - mu_x * mu_x
    var_y = F.conv2d(y * y, window, padding=pad, groups=C) - mu_y * mu_y
    cov = F.conv2d(x * y, window, padding=pad, groups=C) - mu_x * mu_y
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    ssim = (((2 * mu_x * mu_y + c1) * (2 * cov + c2)) / ((mu_x * mu_x + mu_y * mu_y + c1) * (var_x + var_y + c2))).mean()
    return (1 - ssim_weight) * (image - target).abs().mean() + ssim_weight * (1 - ssim)


def map_masked_loss(image, target, mask, ssim_weight=0.2):
    """the masked loss from the operators without mask=: the SSIM map weighted in torch, and a torch L1"""
    w = mask.unsqueeze(-1)
    norm = image.shape[-1] * mask.sum()
    ssim_mean = (ssim(image, target, reduction="none") * w).sum() / norm
    l1 = ((image - target).abs() * w).sum() / norm
    return (1 - ssim_weight) * l1 + ssim_weight * (1 - ssim_mean)


def _mask(args):
    w, h = args.image_size
    return torch.rand(h, w, generator=torch.Generator().manual_seed(args.seed + 1)).to(args.device)


def _inputs(args):
    gen = torch.Generator().manual_seed(args.seed)
    w, h = args.image_size
    target = torch.rand(h, w, args.num_channels, generator=gen)
    image = target + 0.05 * (torch.rand(h, w, args.num_channels, generator=gen) - 0.5)
    return image.to(args.device).requires_grad_(True), target.to(args.device)


def _steps(args, image, target):
    window = torch_window(args.num_channels, args.device)

    def fused():
        image.grad = None
        photometric_loss(image, target, ssim_weight=args.ssim_weight).backward()

    def composed():
        image.grad = None
        torch_photometric_loss(image, target, window, args.ssim_weight).backward()

    return fused, composed


def bench_loss(args):
    image, target = _inputs(args)
    fused, composed = _steps(args, image, target)
    phases = Phases(args)

    def forward():
        return photometric_loss(image, target, ssim_weight=args.ssim_weight)

    def l1_only():
        image.grad = None
        photometric_loss(image, target, ssim_weight=0.0).backward()

    mask = _mask(args)

    def fused_masked():
        image.grad = None
        photometric_loss(image, target, ssim_weight=args.ssim_weight, mask=mask).backward()

    def map_masked():
        image.grad = None
        map_masked_loss(image, target, mask, args.ssim_weight).backward()

    with torch.no_grad():
        phases.run("fused forward", forward)
    phases.run("fused forward+backward", fused)
    phases.run("torch forward+backward", composed)
    phases.run("l1 only", l1_only)
    phases.run("fused masked forward+backward", fused_masked)
    phases.run("map + torch masked forward+backward", map_masked)
    elements = image.numel()
    for name, nbytes in (("fused forward", BYTES_FWD), ("fused forward+backward", BYTES_FWD_BWD)):
        ms = phases.results[name]
        if ms == ms:  # not the profiler's NaN
            rate = nbytes * elements / (ms * 1e-3)
            print(f"{name}: {nbytes} B x {elements} pixel-channels / {ms:.4f} ms = {rate / 1e12:.3f} TB/s "
                  f"({100 * rate / COPY_RATE:.1f}% of the 6.29 TB/s copy rate)")
    return phases.results


def _call_times(f, iters):
    """ms of each of `iters` calls, by device events around every call"""
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in events:
        a.record()
        f()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in events]


def compare(args, warmup=10, iters=50, rounds=2):
    """fused against torch forward+backward: `rounds` alternated rounds of `iters` calls each after `warmup` calls;
    per round the median ms, and the spread between the rounds of one version"""
    image, target = _inputs(args)
    steps = dict(zip(("fused", "torch"), _steps(args, image, target)))
    medians = {name: [] for name in steps}
    for _ in range(rounds):
        for name, f in steps.items():
            for _ in range(warmup):
                f()
            torch.cuda.synchronize()
            medians[name].append(statistics.median(_call_times(f, iters)))
    w, h = args.image_size
    out = dict(image_size=[w, h], channels=args.num_channels, ssim_weight=args.ssim_weight, warmup=warmup, iters=iters,
               rounds=rounds)
    for name, ms in medians.items():
        out[f"{name}_ms_rounds"] = ms
        out[f"{name}_ms"] = statistics.median(ms)
        out[f"{name}_spread_ms"] = max(ms) - min(ms)
    out["ratio_torch_over_fused"] = out["torch_ms"] / out["fused_ms"]
    rate = BYTES_FWD_BWD * image.numel() / (out["fused_ms"] * 1e-3)
    out["fused_compulsory_TBps"] = rate / 1e12
    out["fused_share_of_copy_rate"] = rate / COPY_RATE
    return out


def main():
    args = parse_args()
    results = bench_loss(args)
    if args.json:
        record = compare(args)
        record["phases_ms"] = results
        print(json.dumps(record))
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)
    return results


if __name__ == "__main__":
    main()
