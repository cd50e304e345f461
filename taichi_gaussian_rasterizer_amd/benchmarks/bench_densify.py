"""Densification of a C3-sized table: `plan_densify` + `densify` against the same result composed from the unchanged
ParameterClass methods -- boolean `params[keep]`, the new rows gathered and split in torch, `append_tensors`.

The table: benchmark_scene (1 M rows, SH degree 3: 236 bytes of parameters per row) under VisibilityAwareAdam with its
state populated by one step.  Fixed-seed masks: 5 % prune, 5 % split, 5 % clone, children = 2.  Timed from the masks to
the new ParameterClass, host time and the one read-back included, with the device idle at both ends; the two paths
alternate round by round: `--warmup` calls, `--rounds` rounds of `--iters` calls, median of the round medians, spread =
largest minus smallest round median.  Also reported:
  move     gs_table_move_rows alone (events around the launch inside densify): bytes read + written over time, next to
           the copy rate measured on this chip (COPY_TBPS)
  stats    DensifyStats.update_rows on every row against the index_add_ / index_reduce_ composition
--json PATH writes the record."""
from __future__ import annotations

import json
import math
import statistics
import time

import torch

from .. import _native as nv
from .. import scenes
from ..densify import DensifyStats, densify, plan_densify
from ..optim import ParameterClass, VisibilityAwareAdam
from .bench_train_step import LRS
from .util import FLAGS, make_parser

FLAGS.setdefault("rounds", dict(type=int, default=3))
FLAGS.setdefault("warmup", dict(type=int, default=3))
parse_args = make_parser(("device", "n", "seed", "iters", "degree", "json", "rounds", "warmup"), iters=10)

COPY_TBPS = 6.29  # a plain device-to-device copy on MI355X, read + written bytes over time (bounding roofline)
CHILDREN = 2
SHRINK = 1.6


def make_params(args) -> ParameterClass:
    g, _ = scenes.benchmark_scene(args.n, (2048, 2048), sh_degree=args.degree, seed=args.seed)
    groups = {name: dict(lr=lr, type=kind) for name, lr, kind in LRS}
    params = ParameterClass({k: v.to(args.device) for k, v in g.items()}, groups, optimizer=VisibilityAwareAdam)
    gen = torch.Generator().manual_seed(args.seed + 1)
    for name, t in params.tensors.items():  # one step on every row populates the moments, running_vis, total_weight
        t.grad = (1e-3 * torch.randn(t.shape, generator=gen)).to(args.device)
    rows = torch.arange(args.n, device=args.device)
    params.step(indexes=rows, visibility=(torch.rand(args.n, generator=gen) * 0.9 + 0.05).to(args.device))
    params.zero_grad()
    return params


def make_masks(args):
    r = torch.rand(args.n, generator=torch.Generator().manual_seed(args.seed + 2)).to(args.device)
    return r < 0.05, (r >= 0.05) & (r < 0.10), (r >= 0.10) & (r < 0.15)


def composed(params: ParameterClass, prune, split, clone, noise) -> ParameterClass:
    """the torch composition: what a trainer writes with ParameterClass alone"""
    keep = ~(prune | split)
    new_src = torch.cat([clone.nonzero().flatten(), split.nonzero().flatten().repeat_interleave(CHILDREN)])
    clones = int(clone.sum())
    tensors = params.tensors.detach()
    new = {name: t[new_src] for name, t in tensors.items()}
    parents = new_src[clones:]
    q = torch.nn.functional.normalize(tensors["rotation"][parents], dim=1)
    x, y, z, w = q.unbind(1)
    R = torch.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y,
                     2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x,
                     2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y], dim=1).view(-1, 3, 3)
    offset = tensors["log_scaling"][parents].exp() * noise
    new["position"][clones:] += torch.einsum("mij,mj->mi", R, offset)
    new["log_scaling"][clones:] -= math.log(SHRINK)
    return params[keep].append_tensors(new)


def _wall_ms(f, iters):
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        start = time.perf_counter()
        f()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - start))
    return times


def _summary(rounds):
    return dict(rounds=rounds, ms=statistics.median(rounds), spread_ms=max(rounds) - min(rounds))


def _alternate(paths, args):
    rounds = {name: [] for name in paths}
    for _ in range(args.rounds):
        for name, f in paths.items():
            for _ in range(args.warmup):
                f()
            rounds[name].append(statistics.median(_wall_ms(f, args.iters)))
    return {name: _summary(r) for name, r in rounds.items()}


def bench_surgery(args, params, masks):
    prune, split, clone = masks
    plan = plan_densify(prune, split, clone, children=CHILDREN)
    noise = torch.randn(plan.num_children, 3, generator=torch.Generator().manual_seed(args.seed + 3)).to(args.device)
    out = _alternate({"composition": lambda: composed(params, prune, split, clone, noise),
                      "densify": lambda: densify(params, plan_densify(prune, split, clone, children=CHILDREN),
                                                 noise=noise, shrink=SHRINK),
                      "densify_planned": lambda: densify(params, plan, noise=noise, shrink=SHRINK)}, args)
    a, b = out["composition"], out["densify"]
    out["densify_faster"] = a["ms"] - b["ms"] > max(a["spread_ms"], b["spread_ms"])
    out["plan"] = dict(kept=plan.kept, clones=plan.clones, split_parents=plan.split_parents, rows=plan.rows)

    # the move launch alone
    columns = list(params.tensors.values()) + [t for table in params.tensor_state.values() for t in table.values()]
    state_columns = len(columns) - len(params.tensors)
    row_bytes = [t[0].numel() * t.element_size() for t in columns]
    copied = [plan.rows] * len(params.tensors) + [plan.kept] * state_columns
    moved_bytes = sum(b * (c + plan.rows) for b, c in zip(row_bytes, copied)) + 4 * plan.rows
    nv.timer.reset()
    nv.timer.only, nv.timer.enabled = {"gs_table_move_rows"}, True
    try:
        for _ in range(args.rounds * args.iters):
            densify(params, plan, noise=noise, shrink=SHRINK)
        torch.cuda.synchronize()
        calls, total_ms = nv.timer.summary()["gs_table_move_rows"]
        per_call = sorted(a.elapsed_time(b) for a, b in nv.timer.records["gs_table_move_rows"])
    finally:
        nv.timer.enabled, nv.timer.only = False, None
        nv.timer.reset()
    ms = statistics.median(per_call)
    out["move"] = dict(columns=len(columns), parameter_row_bytes=sum(row_bytes[:len(params.tensors)]),
                       state_row_bytes=sum(row_bytes[len(params.tensors):]), bytes=moved_bytes, calls=calls, ms=ms,
                       min_ms=per_call[0], max_ms=per_call[-1], tbps=moved_bytes / (ms * 1e-3) / 1e12,
                       copy_tbps=COPY_TBPS)
    return out


def bench_stats(args):
    n, dev = args.n, args.device
    gen = torch.Generator().manual_seed(args.seed + 4)
    rows = (torch.rand(n, generator=gen) < 0.8).nonzero().flatten().to(dev)
    v = rows.shape[0]
    grad2d, g2d = torch.randn(v, 7, generator=gen).to(dev), torch.rand(v, 7, generator=gen).to(dev)
    heuristic, visibility = torch.rand(v, 2, generator=gen).to(dev), torch.rand(v, generator=gen).to(dev)
    stats, table = DensifyStats(n, dev), torch.zeros(n, 6, device=dev)

    def torch_update():
        table[:, 0].index_add_(0, rows, (visibility > 0).float())
        table[:, 1].index_add_(0, rows, grad2d[:, :2].norm(dim=1))
        table[:, 2].index_add_(0, rows, heuristic[:, 0])
        table[:, 3].index_add_(0, rows, heuristic[:, 1])
        table[:, 4].index_add_(0, rows, visibility)
        table[:, 5].index_reduce_(0, rows, g2d[:, 4:6].amax(1), "amax")

    out = _alternate({"index_add": torch_update,
                      "update_rows": lambda: stats.update_rows(rows, grad2d=grad2d, heuristic=heuristic,
                                                               visibility=visibility, gaussians2d=g2d)}, args)
    out["listed_rows"] = v
    a, b = out["index_add"], out["update_rows"]
    out["update_faster"] = a["ms"] - b["ms"] > max(a["spread_ms"], b["spread_ms"])
    return out


def bench_densify(args):
    params = make_params(args)
    record = dict(N=args.n, sh_degree=args.degree, children=CHILDREN, warmup=args.warmup, iters=args.iters,
                  rounds=args.rounds, surgery=bench_surgery(args, params, make_masks(args)), stats=bench_stats(args))
    s, m, t = record["surgery"], record["surgery"]["move"], record["stats"]
    print(f"N = {args.n}: {s['plan']['rows']} rows after ({s['plan']['kept']} kept, {s['plan']['clones']} clones, "
          f"{s['plan']['split_parents']} split); {m['columns']} tables, {m['parameter_row_bytes']} + "
          f"{m['state_row_bytes']} bytes per row")
    for name in ("composition", "densify", "densify_planned"):
        print(f"  {name:16s} {s[name]['ms']:8.3f} ms  (spread {s[name]['spread_ms']:.3f}, rounds "
              f"{', '.join(f'{r:.3f}' for r in s[name]['rounds'])})")
    print(f"  densify faster than the composition by more than the spread: {s['densify_faster']}")
    print(f"  gs_table_move_rows {m['ms']:.4f} ms (min {m['min_ms']:.4f}, max {m['max_ms']:.4f}) for "
          f"{m['bytes'] / 1e6:.1f} MB read + written: {m['tbps']:.2f} TB/s (a plain copy: {m['copy_tbps']} TB/s)")
    for name in ("index_add", "update_rows"):
        print(f"  stats {name:12s} {t[name]['ms']:8.3f} ms  (spread {t[name]['spread_ms']:.3f}), "
              f"{t['listed_rows']} listed rows")
    return record


def main():
    args = parse_args()
    record = bench_densify(args)
    print(json.dumps(record))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)
    return record


if __name__ == "__main__":
    main()
