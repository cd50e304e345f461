"""bench_knn runs (at a size that takes seconds) and its record has every figure it reports."""
import math

import pytest

pytestmark = pytest.mark.gpu


def test_bench_knn():
    from taichi_gaussian_rasterizer_amd.benchmarks import bench_knn
    args = bench_knn.parse_args(["--n", "5000", "--small-n", "3000", "--iters", "3", "--rounds", "3", "--warmup", "1"])
    record = bench_knn.bench_knn(args)
    assert record["k"] == 3 and set(record["cases"]) == {"benchmark_scene", "uniform_cube"}
    for case in record["cases"].values():
        assert case["N"] == 5000 and case["small"]["N"] == 3000
        for timing in (case["knn"], case["small"]["cdist"], case["small"]["knn"]):
            assert len(timing["rounds"]) == 3
            assert math.isfinite(timing["ms"]) and timing["ms"] > 0 and timing["spread_ms"] >= 0
        split = case["knn"]["split_ms"]
        assert set(split) == set(bench_knn.LAUNCHES) and all(math.isfinite(ms) and ms > 0 for ms in split.values())
        assert 0 < case["knn"]["scanned_share"] <= 1  # 20 runs: some are neighbours
        assert isinstance(case["small"]["knn_faster"], bool)
        # recorded, not bounded: cdist forms |a|^2 + |b|^2 - 2 a.b, whose float32 error is large next to a small distance
        assert math.isfinite(case["small"]["max_abs_difference"])
