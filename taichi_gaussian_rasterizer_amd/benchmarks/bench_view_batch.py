"""One training iteration over a BATCH of views -- zero_grad, B x (render_gaussians(sparse_grad=True), photometric_loss,
backward) into the same leaves, visible_union, one VisibilityAwareAdam.step -- with the summed gradients read run by
run (optim.fractional.MERGE_RUNS = True: gs_rows_union, gs_rows_find_runs, gs_rows_sum_runs) against the path through
torch.unique and coalesce() (MERGE_RUNS = False), and against the batch taken as a batch (mode "render_views": one
render_views node, one backward of the summed losses, opt.step(*views.visible) on the merged gradient).

Scenes as in bench_train_step: the C3 frame (1 M Gaussians, 2048x2048, SH degree 3) and the same frame plus three times
as many Gaussians behind the camera, rows shuffled.  Batch sizes 2 and 4; the cameras are the benchmark camera moved
sideways, so that the visible sets differ; the record holds every V_b and the size of the union.  The three modes are
timed alternating, round by round: 5 warm-up iterations, 3 rounds of `--iters` (30), median of the round medians, spread
= largest minus smallest round median.  Timed separately: the whole iteration, and the step alone (visible_union +
opt.step between two events).
--json PATH writes the record; --scene NAME runs one scene alone (a profiler run:
rocprofv3 --kernel-trace --stats -- python -m ...bench_view_batch --scene quarter_in_view --iters 10)."""
from __future__ import annotations

import json
import statistics

import torch

from .. import render_gaussians, render_views
from ..data_types import Gaussians3D, RasterConfig
from ..losses import photometric_loss
from ..optim import VisibilityAwareAdam, fractional, visible_union
from .bench_train_step import LRS, make_scene
from .util import make_parser

parse_args = make_parser(("image_size", "device", "n", "seed", "iters", "degree", "scene", "json"), image_size="2048,2048",
                         iters=30)

BATCHES = (2, 4)
SHIFT = 0.01  # sideways step between neighbouring cameras, in scene units (the nearest Gaussians sit at depth 0.1)


def batch_cameras(cam, batch: int):
    """`batch` copies of the camera, moved sideways by multiples of SHIFT around the original"""
    cams = []
    for b in range(batch):
        move = torch.eye(4)
        move[0, 3] = SHIFT * (b - (batch - 1) / 2)
        cams.append(cam.transformed(move))
    return cams


class BatchTrainer:
    def __init__(self, g, cam, device, batch: int):
        self.cams = [c.to(device=device) for c in batch_cameras(cam, batch)]
        self.n = g.position.shape[0]
        self.params = {k: torch.nn.Parameter(v.to(device)) for k, v in g.items()}
        self.opt = VisibilityAwareAdam([dict(params=[self.params[k]], name=k, lr=lr, type=t) for k, lr, t in LRS])
        self.cfg = RasterConfig(compute_visibility=True, compute_point_heuristic=True)
        w, h = cam.image_size
        gen = torch.Generator().manual_seed(1)
        self.targets = [torch.rand(h, w, 3, generator=gen).to(device) for _ in self.cams]
        self.visible, self.union = [], 0

    def iteration(self, merge, step_events=None):
        """merge: the value of MERGE_RUNS for the view-by-view iteration; None: the iteration through render_views"""
        self.opt.zero_grad()
        g = Gaussians3D(**self.params, batch_size=(self.n,))
        if merge is None:
            views = render_views(g, self.cams, self.cfg, use_sh=True)
            sum(photometric_loss(r.image, target) for r, target in zip(views, self.targets)).backward()
            if step_events is not None:
                step_events[0].record()
            self.opt.step(*views.visible)
            if step_events is not None:
                step_events[1].record()
            self.visible, self.union = [r.num_points for r in views], views.num_points
            return
        fractional.MERGE_RUNS = merge
        rs = [render_gaussians(g, cam, self.cfg, use_sh=True, sparse_grad=True) for cam in self.cams]
        for r, target in zip(rs, self.targets):
            photometric_loss(r.image, target).backward()
        if step_events is not None:
            step_events[0].record()
        indexes, visibility = visible_union(rs)
        self.opt.step(indexes, visibility)
        if step_events is not None:
            step_events[1].record()
        self.visible, self.union = [int(r.points_in_view.shape[0]) for r in rs], int(indexes.shape[0])


def _event():
    return torch.cuda.Event(enable_timing=True)


def _times(trainer, merge, iters):
    """(ms per whole iteration, ms per step alone) of `iters` iterations"""
    events = [(_event(), _event(), _event(), _event()) for _ in range(iters)]
    for a, b, s0, s1 in events:
        a.record()
        trainer.iteration(merge, (s0, s1))
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b, _, _ in events], [s0.elapsed_time(s1) for _, _, s0, s1 in events]


def _summary(rounds):
    return dict(rounds=rounds, ms=statistics.median(rounds), spread_ms=max(rounds) - min(rounds))


def bench_batch(args, g, cam, batch: int, warmup=5, rounds=3):
    modes = {"coalesce": False, "merge_runs": True, "render_views": None}
    trainers = {name: BatchTrainer(g, cam, args.device, batch) for name in modes}
    whole = {name: [] for name in modes}
    step = {name: [] for name in modes}
    for _ in range(rounds):
        for name, merge in modes.items():
            for _ in range(warmup):
                trainers[name].iteration(merge)
            torch.cuda.synchronize()
            it, st = _times(trainers[name], merge, args.iters)
            whole[name].append(statistics.median(it))
            step[name].append(statistics.median(st))
    t = trainers["merge_runs"]
    N, C, D = g.position.shape[0], g.feature.shape[1], g.feature.shape[2]
    out = dict(N=N, batch=batch, V=t.visible, union=t.union, channels=C, sh_coefficients=D,
               image_size=list(args.image_size), warmup=warmup, iters=args.iters, rounds=rounds, camera_shift=SHIFT,
               # what autograd's own `grad + new` copies while it accumulates: the b-th backward (b >= 2) writes a new
               # index list and new values holding everything summed so far
               accumulate_copy_bytes=sum((4 * (11 + C * D) + 5 * 8) * sum(t.visible[:b + 1]) for b in range(1, batch)))
    for name in modes:
        out[name] = dict(iteration=_summary(whole[name]), step=_summary(step[name]))
    a, b = out["coalesce"], out["merge_runs"]
    out["step_faster"] = a["step"]["ms"] - b["step"]["ms"] > max(a["step"]["spread_ms"], b["step"]["spread_ms"])
    out["iteration_not_slower"] = b["iteration"]["ms"] - a["iteration"]["ms"] <= a["iteration"]["spread_ms"]
    c = out["render_views"]
    out["render_views_not_slower"] = c["iteration"]["ms"] - b["iteration"]["ms"] <= b["iteration"]["spread_ms"]
    print(f"N = {N}, B = {batch}, V = {t.visible}, union {t.union}: step {a['step']['ms']:.3f} ms coalesce (spread "
          f"{a['step']['spread_ms']:.3f}), {b['step']['ms']:.3f} ms merge_runs (spread {b['step']['spread_ms']:.3f}); "
          f"iteration {a['iteration']['ms']:.3f} (spread {a['iteration']['spread_ms']:.3f}) against "
          f"{b['iteration']['ms']:.3f} (spread {b['iteration']['spread_ms']:.3f}); render_views: step "
          f"{c['step']['ms']:.3f} ms (spread {c['step']['spread_ms']:.3f}), iteration {c['iteration']['ms']:.3f} "
          f"(spread {c['iteration']['spread_ms']:.3f})")
    return out


def bench_scene(args, behind: int):
    g, cam = make_scene(args, behind)
    return {f"batch_{batch}": bench_batch(args, g, cam, batch) for batch in BATCHES}


def main():
    args = parse_args()
    switch = fractional.MERGE_RUNS
    try:
        record = {name: bench_scene(args, behind) for name, behind in (("all_in_view", 0), ("quarter_in_view", 3))
                  if args.scene in ("both", name)}
    finally:
        fractional.MERGE_RUNS = switch
    print(json.dumps(record))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)
    return record


if __name__ == "__main__":
    main()
