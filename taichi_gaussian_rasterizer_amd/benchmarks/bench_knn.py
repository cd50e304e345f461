"""`knn` (gs_knn3d) with k = 3, the initialisation's query, on two point distributions:
  benchmark_scene   the positions of scenes.benchmark_scene(N, (2048, 2048)): a view frustum, dense near the camera
  uniform_cube      N uniform points in the unit cube
Per distribution, at --n points (default 1 M):
  knn       the whole call, `--rounds` rounds of `--iters` calls between two events after `--warmup` calls; median of
            the rounds, spread = largest minus smallest round
  split     device time per launch group from the profiler's kernel table over `--iters` direct gs_knn3d calls:
            reduce (the box partials), codes, sort (every launch of gs_radix_sort_pairs), gather + boxes, query
  scanned   the share of (wave of queries, candidate run) pairs that were scanned rather than skipped by the box test,
            from the counters gs_knn3d leaves at the head of its scratch
and at --small-n points (default 65 536) of the same distribution, a yardstick that is not the code under test:
  cdist     torch.cdist(chunk, points).topk(k + 1, largest=False) over chunks of 4096 rows
  knn       the same call as above; `knn_faster`: by more than the larger spread of the two
--json PATH writes the record."""
from __future__ import annotations

import json
import statistics

import torch
from torch.profiler import ProfilerActivity, profile

from .. import _native as nv
from .. import scenes
from ..neighbours import knn
from .util import FLAGS, make_parser, timed_benchmark

FLAGS.setdefault("rounds", dict(type=int, default=3))
FLAGS.setdefault("warmup", dict(type=int, default=3))
FLAGS.setdefault("small-n", dict(type=int, default=65536, help="points of the comparison with torch.cdist"))
FLAGS.setdefault("k", dict(type=int, default=3))
parse_args = make_parser(("device", "n", "seed", "iters", "json", "rounds", "warmup", "small-n", "k"), iters=10)

CHUNK = 4096
DISTRIBUTIONS = ("benchmark_scene", "uniform_cube")
LAUNCHES = ("reduce", "codes", "sort", "gather_boxes", "query")
_KERNELS = (("knn_bbox", "reduce"), ("knn_codes", "codes"), ("knn_gather", "gather_boxes"), ("knn_query", "query"))


def make_points(name: str, n: int, seed: int, device) -> torch.Tensor:
    if name == "benchmark_scene":
        g, _ = scenes.benchmark_scene(n, (2048, 2048), sh_degree=0, seed=seed)
        return g.position.to(device).contiguous()
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)).to(device)


def cdist_knn(points: torch.Tensor, k: int):
    """the torch composition: chunks of 4096 rows, so that the distance matrix fits in memory"""
    dist, index = [], []
    for start in range(0, points.shape[0], CHUNK):
        d, j = torch.cdist(points[start:start + CHUNK], points).topk(k + 1, largest=False)
        dist.append(d)
        index.append(j)
    return torch.cat(dist), torch.cat(index)


def _rounds(name: str, f, args) -> dict:
    ms = [timed_benchmark(name, f, iters=args.iters, warmup=args.warmup) for _ in range(args.rounds)]
    return dict(rounds=ms, ms=statistics.median(ms), spread_ms=max(ms) - min(ms))


class _DirectCall:
    """gs_knn3d on preallocated buffers: nothing but the library's own launches"""

    def __init__(self, points: torch.Tensor, k: int):
        self.points, self.k, self.n = points, k, int(points.shape[0])
        self.dist2 = torch.empty((self.n, k), dtype=torch.float32, device=points.device)
        self.index = torch.empty((self.n, k), dtype=torch.int32, device=points.device)
        self.bytes = nv.lib().gs_knn3d_scratch_bytes(self.n)
        self.scratch = nv.scratch(self.bytes, points.device)

    def __call__(self):
        nv.check(nv.lib().gs_knn3d(self.n, nv.ptr(self.points), self.k, nv.ptr(self.dist2), nv.ptr(self.index),
                                   nv.ptr(self.scratch), self.bytes, nv.stream()), "gs_knn3d")

    def scanned_share(self) -> float:
        """after a call: scanned (wave, run) pairs over all 4 * runs * (runs - 1)"""
        runs = (self.n + 255) // 256
        if runs < 2:
            return 0.0
        counts = self.scratch[:4 * runs].view(torch.int32)
        return float(counts.sum(dtype=torch.int64)) / (4.0 * runs * (runs - 1))


def launch_split(call: _DirectCall, iters: int) -> dict:
    """ms per call of every launch group, from the profiler's kernel events (sort = every kernel that is not knn's own)"""
    call()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            call()
        torch.cuda.synchronize()
    split = dict.fromkeys(LAUNCHES, 0.0)
    for event in prof.key_averages():
        us = getattr(event, "self_device_time_total", None)
        if us is None:
            us = event.self_cuda_time_total
        if us <= 0:
            continue
        group = next((g for fragment, g in _KERNELS if fragment in event.key), "sort")
        split[group] += us * 1e-3 / iters
    return split


def bench_distribution(name: str, args) -> dict:
    with torch.cuda.device(args.device):
        points = make_points(name, args.n, args.seed, args.device)
        large = _rounds(f"knn {name} N={args.n}", lambda: knn(points, args.k), args)
        call = _DirectCall(points, args.k)
        large["split_ms"] = launch_split(call, args.iters)
        call()
        large["scanned_share"] = call.scanned_share()
        del call

        small_points = make_points(name, args.small_n, args.seed, args.device)
        small = dict(N=args.small_n, chunk=CHUNK,
                     cdist=_rounds(f"cdist+topk {name} N={args.small_n}", lambda: cdist_knn(small_points, args.k), args),
                     knn=_rounds(f"knn {name} N={args.small_n}", lambda: knn(small_points, args.k), args))
        a, b = small["cdist"], small["knn"]
        small["knn_faster"] = a["ms"] - b["ms"] > max(a["spread_ms"], b["spread_ms"])
        # the yardstick computes the same thing: the first neighbour's distance agrees (cdist is not bit-exact)
        d2, _ = knn(small_points, args.k)
        ref, _ = cdist_knn(small_points, args.k)
        small["max_abs_difference"] = float((d2[:, 0].sqrt() - ref[:, 1]).abs().max()) if args.small_n > 1 else 0.0
    return dict(N=args.n, knn=large, small=small)


def bench_knn(args) -> dict:
    record = dict(k=args.k, warmup=args.warmup, iters=args.iters, rounds=args.rounds,
                  cases={name: bench_distribution(name, args) for name in DISTRIBUTIONS})
    for name, case in record["cases"].items():
        big, small = case["knn"], case["small"]
        print(f"{name}: k = {args.k}")
        print(f"  N = {case['N']}: knn {big['ms']:.3f} ms (spread {big['spread_ms']:.3f}, rounds "
              f"{', '.join(f'{r:.3f}' for r in big['rounds'])})")
        print("    per launch: " + ", ".join(f"{g} {big['split_ms'][g]:.3f} ms" for g in LAUNCHES)
              + f"; candidate runs scanned: {100 * big['scanned_share']:.2f} %")
        print(f"  N = {small['N']}: cdist + topk in chunks of {CHUNK} rows {small['cdist']['ms']:.3f} ms (spread "
              f"{small['cdist']['spread_ms']:.3f}), knn {small['knn']['ms']:.3f} ms (spread "
              f"{small['knn']['spread_ms']:.3f}); knn faster by more than the spread: {small['knn_faster']}; "
              f"largest difference of the nearest distance {small['max_abs_difference']:.2e}")
    return record


def main():
    args = parse_args()
    record = bench_knn(args)
    print(json.dumps(record))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)
    return record


if __name__ == "__main__":
    main()
