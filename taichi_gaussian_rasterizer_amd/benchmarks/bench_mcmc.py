"""The MCMC strategy on a C3-sized table: `perturb`, `relocate` and `grow` against the same steps composed in torch.

The table: benchmark_scene (1 M rows, SH degree 3: 236 bytes of parameters per row) under VisibilityAwareAdam with its
state populated by one step (bench_densify's).  Wall time per call, host time included, device idle at both ends; the
paths alternate round by round: `--warmup` calls, `--rounds` rounds of `--iters` calls, median of the round medians,
spread = largest minus smallest round median.
  perturb   gs_mcmc_perturb against R diag(s^2) R^T built as (N, 3, 3) matrices in torch, under three opacity
            distributions: `scene` (benchmark_scene's uniform 0.1 .. 0.9), `mostly_closed` (80 % of the rows above 0.9,
            where the float32 gate is exactly zero) and `open` (every row at 0.002: every gate above 0.5).  The kernel
            alone (events around the launch): the bytes it moves by its traffic model -- 4 per row, 52 more per row
            whose gate is not zero, 4 per position component that changed -- over time, next to gs_table_move_rows'
            rate (MOVE_TBPS), once called back to back (the 68 MB of rows stay in the 256 MiB last-level cache) and
            once with 1 GiB rewritten before every call, which is what a training iteration does to the cache.
  relocate  5 % dead rows, in place, against torch.multinomial + bincount + the series in float64 torch + one index
            assignment per column and state table.  Both paths change the table they are given, call after call.
  grow      5 % new rows against the same draw and series followed by `append_tensors`.
--json PATH writes the record."""
from __future__ import annotations

import json
import math
import statistics

import torch

from .. import _native as nv
from ..mcmc import grow, perturb, relocate
from ..optim import ParameterClass
from .bench_densify import _alternate, make_params
from .util import FLAGS, make_parser

FLAGS.setdefault("rounds", dict(type=int, default=3))
FLAGS.setdefault("warmup", dict(type=int, default=3))
parse_args = make_parser(("device", "n", "seed", "iters", "degree", "json", "rounds", "warmup"), iters=10)

MOVE_TBPS = 5.17  # gs_table_move_rows on this chip (profiles/densify/bench.txt)
EVICT_BYTES = 1 << 30  # four times the 256 MiB last-level cache
LR, NOISE_LR, K, X0 = 1.6e-6, 5e5, 100.0, 0.995
MIN_OPACITY, N_MAX = 0.005, 51
DEAD_FRACTION = GROW_FRACTION = 0.05


# ----------------------------------------------------------------------------------------------- the torch compositions
def rotation_matrices(rotation):
    x, y, z, w = torch.nn.functional.normalize(rotation, dim=1).unbind(1)
    return torch.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y,
                        2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x,
                        2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y], dim=1).view(-1, 3, 3)


def torch_perturb(table, noise, scale):
    R = rotation_matrices(table["rotation"])
    M = R * table["log_scaling"].exp().unsqueeze(1)          # R S
    covariance = M @ M.transpose(1, 2)                        # R S S^T R^T
    gate = torch.sigmoid(K * ((1 - torch.sigmoid(table["alpha_logit"])) - X0))
    table["position"].add_(torch.bmm(covariance, (noise * gate * scale).unsqueeze(-1)).squeeze(-1))


_BINOMIALS = {}


def binomials(device):
    if device not in _BINOMIALS:
        _BINOMIALS[device] = torch.tensor([[float(math.comb(n, k)) for k in range(N_MAX + 1)]
                                           for n in range(N_MAX + 1)], dtype=torch.float64, device=device)
    return _BINOMIALS[device]


def torch_values(opacity, log_scaling, ratio):
    """the correction of rows that become `ratio` rows, float64 in torch; the double sum collapsed over i
    (sum_{i > k} C(i - 1, k) = C(n, k + 1)), which keeps the temporaries at (rows, 51)"""
    o, n = opacity.double(), ratio.clamp(max=N_MAX)
    x = (1 - (1 - o) ** (1 / n.double())).clamp(MIN_OPACITY, 1 - 2.0 ** -23)
    k = torch.arange(N_MAX, device=o.device)
    terms = binomials(o.device)[n][:, 1:] * (-1.0) ** k * x.unsqueeze(1) ** (k + 1) / (k + 1).double().sqrt()
    denom = terms.sum(1)
    return (x / (1 - x)).log().float(), log_scaling + (o / denom).log().float().unsqueeze(1)


def torch_draw(opacity, count):
    src = torch.multinomial(opacity, count, replacement=True)
    return src, torch.bincount(src, minlength=opacity.shape[0])


def torch_relocate(params: ParameterClass, dead):
    tensors = {name: t.detach() for name, t in params.tensors.items()}
    opacity = torch.sigmoid(tensors["alpha_logit"]).flatten()
    dead_rows = dead.nonzero().flatten()
    src, copies = torch_draw(opacity.masked_fill(dead, 0), dead_rows.shape[0])
    alpha_logit, log_scaling = torch_values(opacity[src], tensors["log_scaling"][src], copies[src] + 1)
    for name, t in tensors.items():
        t[dead_rows] = t[src]
    for rows in (dead_rows, src):
        tensors["alpha_logit"][rows] = alpha_logit.unsqueeze(1)
        tensors["log_scaling"][rows] = log_scaling
    for table in params.tensor_state.values():
        for t in table.values():
            t[dead_rows] = 0
            t[src] = 0


def torch_grow(params: ParameterClass, count):
    tensors = {name: t.detach() for name, t in params.tensors.items()}
    opacity = torch.sigmoid(tensors["alpha_logit"]).flatten()
    src, copies = torch_draw(opacity, count)
    alpha_logit, log_scaling = torch_values(opacity[src], tensors["log_scaling"][src], copies[src] + 1)
    new = {name: t[src] for name, t in tensors.items()}
    new["alpha_logit"], new["log_scaling"] = alpha_logit.unsqueeze(1), log_scaling
    grown = params.append_tensors(new)
    grown.tensors["alpha_logit"].detach()[src] = alpha_logit.unsqueeze(1)
    grown.tensors["log_scaling"].detach()[src] = log_scaling
    return grown


# ---------------------------------------------------------------------------------------------------------- the parts
def opacity_cases(args, scene_alpha_logit):
    n, dev = args.n, args.device
    u = torch.rand(n, generator=torch.Generator().manual_seed(args.seed + 5)).to(dev)
    closed = 0.9 + 0.0999 * u * 1.25                      # the 80 % with u < 0.8: 0.9 .. 0.9999
    rest = 1e-3 + (0.9 - 1e-3) * (u - 0.8) * 5
    mostly_closed = torch.where(u < 0.8, closed, rest).clamp(1e-3, 0.9999)
    return {"scene": scene_alpha_logit.detach().clone(),
            "mostly_closed": torch.logit(mostly_closed).view(n, 1),
            "open": torch.full((n, 1), math.log(0.002 / 0.998), device=dev)}


def kernel_ms(name, f, calls, evict=None):
    """the launch alone, between events; `evict`: a buffer larger than the last-level cache, rewritten before every
    call (outside the events), so that the launch reads its rows from memory as it does inside a training iteration"""
    nv.timer.reset()
    nv.timer.only, nv.timer.enabled = {name}, True
    try:
        for _ in range(calls):
            if evict is not None:
                evict.add_(1)
            f()
        torch.cuda.synchronize()
        per_call = sorted(a.elapsed_time(b) for a, b in nv.timer.records[name])
    finally:
        nv.timer.enabled, nv.timer.only = False, None
        nv.timer.reset()
    return dict(calls=len(per_call), ms=statistics.median(per_call), min_ms=per_call[0], max_ms=per_call[-1])


def bench_perturb(args, params):
    n, dev = args.n, args.device
    scale = LR * NOISE_LR
    noise = torch.randn(n, 3, generator=torch.Generator().manual_seed(args.seed + 6)).to(dev)
    base = {name: params.tensors[name].detach().clone() for name in ("position", "log_scaling", "rotation")}
    evict_buffer = torch.zeros(EVICT_BYTES // 4, dtype=torch.int32, device=dev)
    out = {}
    for case, alpha_logit in opacity_cases(args, params.tensors["alpha_logit"]).items():
        table = {**{name: t.clone() for name, t in base.items()}, "alpha_logit": alpha_logit}
        other = {name: t.clone() for name, t in table.items()}
        record = _alternate({"torch": lambda: torch_perturb(other, noise, scale),
                             "perturb": lambda: perturb(table, LR, noise=noise, noise_lr=NOISE_LR, k=K, x0=X0)}, args)
        a, b = record["torch"], record["perturb"]
        record["perturb_faster"] = a["ms"] - b["ms"] > max(a["spread_ms"], b["spread_ms"])
        # the traffic model, from one call on a fresh copy of the positions
        table["position"].copy_(base["position"])
        gate = torch.sigmoid(K * ((1 - torch.sigmoid(alpha_logit.flatten())) - X0))
        perturb(table, LR, noise=noise, noise_lr=NOISE_LR, k=K, x0=X0)
        open_rows = int((gate != 0).sum())
        changed = int((table["position"].view(torch.int32) != base["position"].view(torch.int32)).sum())
        moved_bytes = 4 * n + 52 * open_rows + 4 * changed
        for key, evict in (("kernel", None), ("kernel_cold", evict_buffer)):
            kernel = kernel_ms("gs_mcmc_perturb", lambda: perturb(table, LR, noise=noise, noise_lr=NOISE_LR, k=K, x0=X0),
                               args.rounds * args.iters, evict)
            kernel.update(open_rows=open_rows, changed_components=changed, bytes=moved_bytes,
                          bytes_per_row=moved_bytes / n, tbps=moved_bytes / (kernel["ms"] * 1e-3) / 1e12,
                          move_tbps=MOVE_TBPS)
            record[key] = kernel
        out[case] = record
    return out


def bench_relocate(args, params):
    n, dev = args.n, args.device
    dead = (torch.rand(n, generator=torch.Generator().manual_seed(args.seed + 7)) < DEAD_FRACTION).to(dev)
    ours, theirs = (params.apply(lambda t: t.detach().clone()) for _ in range(2))
    out = _alternate({"composition": lambda: torch_relocate(theirs, dead),
                      "relocate": lambda: relocate(ours, dead, min_opacity=MIN_OPACITY)}, args)
    a, b = out["composition"], out["relocate"]
    out["relocate_faster"] = a["ms"] - b["ms"] > max(a["spread_ms"], b["spread_ms"])
    out["dead_rows"] = int(dead.sum())
    out["tables"] = len(params.tensors) + sum(len(table) for table in params.tensor_state.values())
    return out


def bench_grow(args, params):
    count = int(GROW_FRACTION * args.n)
    out = _alternate({"composition": lambda: torch_grow(params, count),
                      "grow": lambda: grow(params, count, min_opacity=MIN_OPACITY)}, args)
    a, b = out["composition"], out["grow"]
    out["grow_faster"] = a["ms"] - b["ms"] > max(a["spread_ms"], b["spread_ms"])
    out["new_rows"] = count
    return out


def bench_mcmc(args):
    params = make_params(args)
    record = dict(N=args.n, sh_degree=args.degree, warmup=args.warmup, iters=args.iters, rounds=args.rounds,
                  lr=LR, noise_lr=NOISE_LR, perturb=bench_perturb(args, params), relocate=bench_relocate(args, params),
                  grow=bench_grow(args, params))
    print(f"N = {args.n}, SH degree {args.degree}")
    for case, p in record["perturb"].items():
        k, c = p["kernel"], p["kernel_cold"]
        print(f"  perturb [{case}]: torch {p['torch']['ms']:.3f} ms (spread {p['torch']['spread_ms']:.3f}), perturb "
              f"{p['perturb']['ms']:.3f} ms (spread {p['perturb']['spread_ms']:.3f}); {k['open_rows']} rows with a gate, "
              f"{k['bytes_per_row']:.1f} bytes per row; kernel alone, rows in cache: {k['ms']:.4f} ms (min "
              f"{k['min_ms']:.4f}, max {k['max_ms']:.4f}) = {k['tbps']:.2f} TB/s; cache evicted before each call: "
              f"{c['ms']:.4f} ms (min {c['min_ms']:.4f}, max {c['max_ms']:.4f}) = {c['tbps']:.2f} TB/s "
              f"(move: {k['move_tbps']} TB/s)")
    for part, ours in (("relocate", "relocate"), ("grow", "grow")):
        r = record[part]
        print(f"  {part}: composition {r['composition']['ms']:.3f} ms (spread {r['composition']['spread_ms']:.3f}), "
              f"{ours} {r[ours]['ms']:.3f} ms (spread {r[ours]['spread_ms']:.3f}); faster by more than the spread: "
              f"{r[ours + '_faster']}")
    return record


def main():
    args = parse_args()
    record = bench_mcmc(args)
    print(json.dumps(record))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)
    return record


if __name__ == "__main__":
    main()
