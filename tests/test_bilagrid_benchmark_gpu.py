"""benchmarks/bench_bilagrid.py at 256 x 256 with 3 iterations: the record holds every figure, and the figures are finite."""
import math

import pytest

pytestmark = pytest.mark.gpu


def test_bench_bilagrid_record():
    from taichi_gaussian_rasterizer_amd.benchmarks import bench_bilagrid
    args = bench_bilagrid.parse_args(["--bilagrid_size", "256,256", "--iters", "3", "--warmup", "1"])
    record = bench_bilagrid.bench_bilagrid(args)
    assert record["iters"] == 3 and record["rounds"] == 3 and len(record["cases"]) == 2
    assert [tuple(case["grid"]) for case in record["cases"]] == [(8, 16, 16), (1, 1, 1)]
    for case in record["cases"]:
        assert (case["height"], case["width"], case["pixels"]) == (256, 256, 65536)
        for part, per_pixel in (("forward", 24), ("forward_backward", 60)):
            r = case[part]
            assert r["bytes"] == per_pixel * 65536 and isinstance(r["fused_faster"], bool)
            for path in ("fused", "torch", "stream"):
                assert len(r[path]["rounds"]) == 3
                assert all(math.isfinite(v) and v > 0 for v in r[path]["rounds"] + [r[path]["ms"]])
                assert math.isfinite(r[path]["spread_ms"]) and r[path]["spread_ms"] >= 0
            for key in ("fused_tbps", "stream_tbps", "ratio_to_stream", "speedup"):
                assert math.isfinite(r[key]) and r[key] > 0, key
