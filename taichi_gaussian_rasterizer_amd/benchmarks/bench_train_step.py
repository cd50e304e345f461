"""One training iteration -- zero_grad, render_gaussians (visibility and heuristics on), photometric_loss, backward,
VisibilityAwareAdam.step -- with dense parameter gradients against render_gaussians(sparse_grad=True).

Two scenes: the C3 frame (1 M Gaussians, 2048x2048, SH degree 3: nearly everything is in view), and the same frame plus
three times as many Gaussians behind the camera, rows shuffled, so that about a quarter is in view.  The two modes are
timed alternating, round by round; per mode the record holds the median iteration, the spread between its rounds, the
backward's stage times from the frame call's stage events and torch.cuda.max_memory_allocated over the backward, next
to the modelled gradient bytes: 4 (11 + C D) N dense, 4 (11 + C D) V + 8 V sparse.
--json PATH writes the record; --scene NAME runs one scene alone (a profiler run of the quarter-in-view iteration:
rocprofv3 --kernel-trace --stats -- python -m ...bench_train_step --scene quarter_in_view --iters 10)."""
from __future__ import annotations

import json
import statistics

import torch

from .. import _native as nv
from .. import render_gaussians, scenes
from ..data_types import Gaussians3D, RasterConfig
from ..losses import photometric_loss
from ..optim import VisibilityAwareAdam
from .util import make_parser

parse_args = make_parser(("image_size", "device", "n", "seed", "iters", "degree", "scene", "json"), image_size="2048,2048",
                         iters=30)

LRS = (("position", 1e-5, "vector"), ("log_scaling", 1e-4, "vector"), ("rotation", 1e-4, "vector"),
       ("alpha_logit", 1e-3, "scalar"), ("feature", 1e-4, "scalar"))


def make_scene(args, behind: int):
    """the benchmark frame plus `behind` times as many Gaussians mirrored behind the camera, rows shuffled"""
    g, cam = scenes.benchmark_scene(args.n, args.image_size, sh_degree=args.degree, seed=args.seed)
    if behind:
        parts = [g]
        for k in range(behind):
            extra, _ = scenes.benchmark_scene(args.n, args.image_size, sh_degree=args.degree, seed=args.seed + 1 + k)
            parts.append(extra.replace(position=extra.position * torch.tensor([1.0, 1.0, -1.0])))
        for part in parts[1:]:
            g = g.concat(part)
        perm = torch.randperm(g.position.shape[0], generator=torch.Generator().manual_seed(args.seed + 99))
        g = g[perm].contiguous()
    return g, cam


class Trainer:
    def __init__(self, g, cam, device, sparse: bool):
        self.sparse, self.cam = sparse, cam.to(device=device)
        self.n = g.position.shape[0]
        self.params = {k: torch.nn.Parameter(v.to(device)) for k, v in g.items()}
        self.opt = VisibilityAwareAdam([dict(params=[self.params[k]], name=k, lr=lr, type=t) for k, lr, t in LRS])
        self.cfg = RasterConfig(compute_visibility=True, compute_point_heuristic=True)
        w, h = cam.image_size
        self.target = torch.rand(h, w, 3, generator=torch.Generator().manual_seed(1)).to(device)
        self.visible = 0
        self.backward_peak = 0

    def iteration(self, measure_peak: bool = False):
        self.opt.zero_grad()
        g = Gaussians3D(**self.params, batch_size=(self.n,))
        r = render_gaussians(g, self.cam, self.cfg, use_sh=True, sparse_grad=self.sparse)
        loss = photometric_loss(r.image, self.target)
        if measure_peak:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
        loss.backward()
        if measure_peak:
            torch.cuda.synchronize()
            self.backward_peak = torch.cuda.max_memory_allocated() - before
        self.opt.step(r.points_in_view, r.point_visibility)
        self.visible = int(r.points_in_view.shape[0])


def _times(trainer, iters):
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in events:
        a.record()
        trainer.iteration()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in events]


def _stage_times(trainer, iters):
    """ms per iteration of the backward's stages, from the frame call's stage events"""
    nv.timer.reset()
    nv.timer.only = set(nv.FRAME_BWD_STAGES)
    nv.timer.enabled = True
    for _ in range(iters):
        trainer.iteration()
    torch.cuda.synchronize()
    nv.timer.enabled = False
    out = {name: total / max(calls, 1) for name, (calls, total) in nv.timer.summary().items()}
    nv.timer.reset()
    nv.timer.only = None
    return out


def bench_scene(args, behind: int, warmup=5, rounds=3):
    g, cam = make_scene(args, behind)
    trainers = {"dense": Trainer(g, cam, args.device, False), "sparse": Trainer(g, cam, args.device, True)}
    rounds_ms = {name: [] for name in trainers}
    for _ in range(rounds):
        for name, t in trainers.items():
            for _ in range(warmup):
                t.iteration()
            torch.cuda.synchronize()
            rounds_ms[name].append(statistics.median(_times(t, args.iters)))
    N, C, D = g.position.shape[0], g.feature.shape[1], g.feature.shape[2]
    V = trainers["sparse"].visible
    row = 4 * (11 + C * D)
    out = dict(N=N, V=V, channels=C, sh_coefficients=D, image_size=list(args.image_size), warmup=warmup,
               iters=args.iters, rounds=rounds, grad_bytes_dense=row * N, grad_bytes_sparse=row * V + 8 * V)
    for name, t in trainers.items():
        ms = rounds_ms[name]
        t.iteration(measure_peak=True)
        out[name] = dict(iteration_ms_rounds=ms, iteration_ms=statistics.median(ms), spread_ms=max(ms) - min(ms),
                         backward_stage_ms=_stage_times(t, 10), backward_peak_bytes=int(t.backward_peak))
    out["sparse_over_dense"] = out["sparse"]["iteration_ms"] / out["dense"]["iteration_ms"]
    print(f"N = {N}, V = {V}: dense {out['dense']['iteration_ms']:.3f} ms (spread {out['dense']['spread_ms']:.3f}), "
          f"sparse {out['sparse']['iteration_ms']:.3f} ms (spread {out['sparse']['spread_ms']:.3f}); backward peak "
          f"{out['dense']['backward_peak_bytes'] / 2**20:.0f} MiB dense, "
          f"{out['sparse']['backward_peak_bytes'] / 2**20:.0f} MiB sparse")
    return out


def main():
    args = parse_args()
    record = {name: bench_scene(args, behind) for name, behind in (("all_in_view", 0), ("quarter_in_view", 3))
              if args.scene in ("both", name)}
    print(json.dumps(record))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)
    return record


if __name__ == "__main__":
    main()
