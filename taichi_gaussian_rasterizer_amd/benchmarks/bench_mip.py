"""Mip-Splatting's 3D smoothing filter on the C3 frame (1 M Gaussians, 2048 x 2048, SH degree 3) against the same steps
composed in torch.

Wall time per call, host time included, device idle at both ends; the paths alternate round by round: `--warmup` calls,
`--rounds` rounds of `--iters` calls, median of the round medians, spread = largest minus smallest round median.
  sampling_rate  the scene's positions against `--cameras` random cameras on a sphere around them (sizes, focal lengths
                 and planes differ), and the same result composed in torch, one pass over N per camera.  The launch alone
                 (events around it): (point, camera) pairs per second and the share of the chip's float32 VALU rate that
                 the VALU_PER_PAIR instructions of the loop body (counted in the assembly, the division's branch left
                 out) amount to.
  smooth3d       forward, dense backward and row-compact backward (the rows of the frame's points_in_view) against
                 the formulas written plainly in torch with autograd.  The launches alone, called back to back and with
                 1 GiB rewritten before every call: bytes by the shapes (36 per row forward, 52 dense backward, 60 per
                 listed row in the row form) over time, next to the streaming rates of gs_mcmc_perturb and
                 gs_table_move_rows on this chip.
  iteration      render_gaussians(sparse_grad=True) + photometric_loss + backward on the frame: with smooth3d in front,
                 without it, and with the torch composition in front (whose gradients reach the leaves dense).
--json PATH writes the record."""
from __future__ import annotations

import json
import math

import torch

from .. import scenes
from ..data_types import RasterConfig
from ..losses import photometric_loss
from ..mip import pack_cameras, sampling_rate, smooth3d, smooth_gaussians
from ..perspective.params import CameraParams
from ..renderer import render_gaussians
from .bench_densify import _alternate
from .bench_mcmc import EVICT_BYTES, MOVE_TBPS, kernel_ms
from .util import FLAGS, make_parser

FLAGS.setdefault("rounds", dict(type=int, default=3))
FLAGS.setdefault("warmup", dict(type=int, default=3))
FLAGS.setdefault("cameras", dict(type=int, default=256, help="cameras of the sampling-rate sweep"))
parse_args = make_parser(("image_size", "device", "n", "seed", "iters", "degree", "json", "rounds", "warmup", "cameras"),
                         image_size="2048,2048", iters=10)

PERTURB_TBPS = 2.74        # gs_mcmc_perturb, every gate open, cache evicted (profiles/mcmc/bench.txt)
VALU_PER_PAIR = 34         # VALU instructions of the sweep's loop body per (point, camera) pair without the division:
#                            17 v_mul_f32 + 11 v_add_f32 (the three rows, u, v, the four bounds) + 6 v_cmp, counted in
#                            the assembly (profiles/mip/isa_identity.txt)
VALU_LANE_RATE = 157.3e12 / 2  # float32 lane-instructions per second: the vector peak counts a fused multiply-add as 2
FWD_BYTES, BWD_BYTES, ROW_BYTES = 36, 52, 60


def torch_smooth3d(log_scaling, alpha_logit, filter3d):
    """the formulas written plainly: what a trainer composes without the operator"""
    f2 = filter3d.reshape(-1, 1) ** 2
    scale2 = torch.exp(2 * log_scaling)
    smoothed2 = scale2 + f2
    c = torch.sqrt(torch.prod(scale2 / smoothed2, dim=1, keepdim=True))
    opacity = torch.sigmoid(alpha_logit) * c
    return 0.5 * torch.log(smoothed2), torch.log(opacity / (1 - opacity))


def random_cameras(positions, count, seed, device):
    """`count` cameras on a sphere around the finite positions' centre, looking at it"""
    gen = torch.Generator().manual_seed(seed)
    centre = positions.mean(0).cpu()
    radius = float((positions.cpu() - centre).norm(dim=1).median())
    cams = []
    for _ in range(count):
        direction = torch.nn.functional.normalize(torch.randn(3, generator=gen), dim=0)
        eye = centre + direction * radius * float(1.0 + 2.0 * torch.rand((), generator=gen))
        z = torch.nn.functional.normalize(centre - eye, dim=0)
        x = torch.nn.functional.normalize(torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0]), z), dim=0)
        R = torch.stack([x, torch.linalg.cross(z, x), z])
        T = torch.eye(4)
        T[:3, :3], T[:3, 3] = R, -R @ eye
        w, h = (int(v) for v in torch.randint(480, 2049, (2,), generator=gen))
        fx = float(w) * float(0.5 + 1.5 * torch.rand((), generator=gen))
        cams.append(CameraParams(projection=torch.tensor([fx, fx * 1.05, w / 2, h / 2]), T_camera_world=T,
                                 near_plane=0.01 * radius, far_plane=10.0 * radius, image_size=(w, h)).to(device=device))
    return cams


def torch_sampling_rate(positions, table, records):
    """one pass over N per camera, in torch; records = table.tolist(), read back once like pack_cameras' inputs"""
    rate = torch.zeros(positions.shape[0], device=positions.device)
    seen = torch.zeros(positions.shape[0], dtype=torch.int32, device=positions.device)
    poses = table[:, :12].view(-1, 3, 4)
    for T, cam in zip(poses, records):
        p = positions @ T[:, :3].T + T[:, 3]
        z = p[:, 2]
        u, v = cam[12] * p[:, 0] + cam[14] * z, cam[13] * p[:, 1] + cam[15] * z
        valid = ((z >= cam[20]) & (z <= cam[21]) & (cam[16] * z <= u) & (u <= cam[17] * z) & (cam[18] * z <= v) &
                 (v <= cam[19] * z))
        rate = torch.where(valid, torch.maximum(rate, cam[22] / z), rate)
        seen += valid
    return rate, seen


def bench_sampling_rate(args, positions):
    n, dev = args.n, args.device
    table = pack_cameras(random_cameras(positions, args.cameras, args.seed + 11, dev))
    records = table.cpu().tolist()
    out = _alternate({"torch": lambda: torch_sampling_rate(positions, table, records),
                      "sampling_rate": lambda: sampling_rate(positions, table)}, args)
    a, b = out["torch"], out["sampling_rate"]
    out["sampling_rate_faster"] = a["ms"] - b["ms"] > max(a["spread_ms"], b["spread_ms"])
    rate, seen = sampling_rate(positions, table)
    pairs = n * args.cameras
    kernel = kernel_ms("gs_mip_sampling_rate", lambda: sampling_rate(positions, table), args.rounds * args.iters)
    seconds = kernel["ms"] * 1e-3
    kernel.update(pairs=pairs, pairs_per_second=pairs / seconds, valid_pairs=int(seen.sum()),
                  valu_per_pair=VALU_PER_PAIR, valu_share=pairs * VALU_PER_PAIR / seconds / VALU_LANE_RATE)
    out.update(kernel=kernel, cameras=args.cameras, seen_rows=int((seen > 0).sum()),
               mean_cameras_per_seen_row=float(seen.sum()) / max(int((seen > 0).sum()), 1),
               seen_equal_torch=bool(torch.equal(seen, torch_sampling_rate(positions, table, records)[1])))
    return out, rate, seen


def bench_smooth3d(args, g, filter3d, rows):
    n, dev, v = args.n, args.device, int(rows.shape[0])
    l, a = g.log_scaling.detach(), g.alpha_logit.detach()
    gl, ga = torch.randn_like(l), torch.randn_like(a)
    idx = rows.view(1, v)
    sparse_l = torch.sparse_coo_tensor(idx, gl[rows].contiguous(), l.shape, is_coalesced=True)
    sparse_a = torch.sparse_coo_tensor(idx, ga[rows].contiguous(), a.shape, is_coalesced=True)

    def run(fn, grads):
        ll, aa = l.clone().requires_grad_(True), a.clone().requires_grad_(True)
        out = fn(ll, aa, filter3d)
        if grads is not None:
            torch.autograd.backward(out, grads)
        return ll.grad, aa.grad

    out = _alternate({"torch_forward": lambda: run(torch_smooth3d, None), "forward": lambda: run(smooth3d, None),
                      "torch_forward_backward": lambda: run(torch_smooth3d, [gl, ga]),
                      "forward_backward": lambda: run(smooth3d, [gl, ga]),
                      "forward_backward_rows": lambda: run(smooth3d, [sparse_l, sparse_a])}, args)
    got = run(smooth3d, [sparse_l, sparse_a])
    assert got[0].is_sparse and got[1].is_sparse and got[0]._nnz() == v
    evict = torch.zeros(EVICT_BYTES // 4, dtype=torch.int32, device=dev)
    calls = args.rounds * args.iters
    for name, fn, count, per_row in (("gs_smooth3d_fwd", lambda: run(smooth3d, None), n, FWD_BYTES),
                                     ("gs_smooth3d_bwd", lambda: run(smooth3d, [gl, ga]), n, BWD_BYTES),
                                     ("gs_smooth3d_bwd_rows", lambda: run(smooth3d, [sparse_l, sparse_a]), v, ROW_BYTES)):
        for key, buffer in (("kernel", None), ("kernel_cold", evict)):
            kernel = kernel_ms(name, fn, calls, buffer)
            kernel.update(rows=count, bytes=count * per_row, tbps=count * per_row / (kernel["ms"] * 1e-3) / 1e12,
                          perturb_tbps=PERTURB_TBPS, move_tbps=MOVE_TBPS)
            out[f"{name}_{key}"] = kernel
    out.update(N=n, V=v)
    return out


def bench_iteration(args, g, cam, filter3d):
    h, w = cam.image_size[1], cam.image_size[0]
    target = torch.rand(h, w, 3, generator=torch.Generator().manual_seed(1)).to(args.device)
    cfg = RasterConfig()
    leaves = g.detach().clone().requires_grad_(True)
    state = {}
    # torch's elementwise backwards take the frame's sparse gradients where this torch supports the products involved
    # and make them dense on the way; where it does not, the composition renders with dense gradients from the start
    torch_sparse = True
    try:
        probe = leaves.replace(**dict(zip(("log_scaling", "alpha_logit"),
                                          torch_smooth3d(leaves.log_scaling, leaves.alpha_logit, filter3d))))
        render_gaussians(probe, cam, cfg, use_sh=True, sparse_grad=True).image.sum().backward()
    except (RuntimeError, NotImplementedError):
        torch_sparse = False

    def iteration(front):
        for _, t in leaves.items():
            t.grad = None
        if front == "smooth3d":
            shown = smooth_gaussians(leaves, filter3d)
        elif front == "torch":
            shown = leaves.replace(**dict(zip(("log_scaling", "alpha_logit"),
                                              torch_smooth3d(leaves.log_scaling, leaves.alpha_logit, filter3d))))
        else:
            shown = leaves
        r = render_gaussians(shown, cam, cfg, use_sh=True, sparse_grad=torch_sparse or front != "torch")
        photometric_loss(r.image, target).backward()
        state[front] = (leaves.log_scaling.grad.is_sparse, int(r.points_in_view.shape[0]))

    out = _alternate({"smooth3d": lambda: iteration("smooth3d"), "none": lambda: iteration("none"),
                      "torch": lambda: iteration("torch")}, args)
    out["log_scaling_grad_sparse"] = {front: sparse for front, (sparse, _) in state.items()}
    out["torch_front_takes_sparse_gradients"] = torch_sparse
    out["visible"] = state["smooth3d"][1]
    out["smooth3d_cost_ms"] = out["smooth3d"]["ms"] - out["none"]["ms"]
    out["torch_cost_ms"] = out["torch"]["ms"] - out["none"]["ms"]
    return out


def bench_mip(args):
    dev = args.device
    g, cam = scenes.benchmark_scene(args.n, args.image_size, sh_degree=args.degree, seed=args.seed)
    g, cam = g.to(dev), cam.to(device=dev)
    rate_record, rate, seen = bench_sampling_rate(args, g.position)
    filter3d = torch.where(seen > 0, math.sqrt(0.2) / rate, torch.zeros_like(rate))
    filter3d = torch.where(seen > 0, filter3d, filter3d.max())
    with torch.no_grad():
        rows = render_gaussians(g, cam, RasterConfig(), use_sh=True).points_in_view.clone()
    record = dict(N=args.n, sh_degree=args.degree, image_size=list(args.image_size), warmup=args.warmup,
                  iters=args.iters, rounds=args.rounds, sampling_rate=rate_record,
                  smooth3d=bench_smooth3d(args, g, filter3d, rows), iteration=bench_iteration(args, g, cam, filter3d))
    s, k = record["sampling_rate"], record["sampling_rate"]["kernel"]
    print(f"N = {args.n}, {args.cameras} cameras, frame {args.image_size[0]}x{args.image_size[1]}, SH degree {args.degree}")
    print(f"  sampling_rate: torch {s['torch']['ms']:.3f} ms (spread {s['torch']['spread_ms']:.3f}), sampling_rate "
          f"{s['sampling_rate']['ms']:.3f} ms (spread {s['sampling_rate']['spread_ms']:.3f}); kernel alone {k['ms']:.4f} ms "
          f"= {k['pairs_per_second'] / 1e9:.1f} G pairs/s = {100 * k['valu_share']:.1f} % of the VALU rate at "
          f"{k['valu_per_pair']} instructions per pair; {s['seen_rows']} rows seen, by "
          f"{s['mean_cameras_per_seen_row']:.1f} cameras each")
    m = record["smooth3d"]
    for name in ("torch_forward", "forward", "torch_forward_backward", "forward_backward", "forward_backward_rows"):
        print(f"  smooth3d {name}: {m[name]['ms']:.3f} ms (spread {m[name]['spread_ms']:.3f})")
    for name in ("gs_smooth3d_fwd", "gs_smooth3d_bwd", "gs_smooth3d_bwd_rows"):
        hot, cold = m[name + "_kernel"], m[name + "_kernel_cold"]
        print(f"  {name}: {hot['rows']} rows, {hot['bytes'] / 1e6:.1f} MB; back to back {hot['ms']:.4f} ms = "
              f"{hot['tbps']:.2f} TB/s; cache evicted {cold['ms']:.4f} ms = {cold['tbps']:.2f} TB/s (perturb "
              f"{PERTURB_TBPS}, move {MOVE_TBPS} TB/s)")
    it = record["iteration"]
    for name in ("smooth3d", "none", "torch"):
        print(f"  iteration, {name} in front: {it[name]['ms']:.3f} ms (spread {it[name]['spread_ms']:.3f}); "
              f"log_scaling.grad sparse: {it['log_scaling_grad_sparse'][name]}")
    return record


def main():
    args = parse_args()
    record = bench_mip(args)
    print(json.dumps(record))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)
    return record


if __name__ == "__main__":
    main()
