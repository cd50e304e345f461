"""benchmarks/bench_envmap.py at 256 x 256 with 3 iterations: the record holds every figure, the figures are finite, and
the byte counts are the stated per-pixel and per-texel formulas."""
import math

import pytest

pytestmark = pytest.mark.gpu


def _finite_path(path):
    assert len(path["rounds"]) == 3
    assert all(math.isfinite(v) and v > 0 for v in path["rounds"] + [path["ms"]])
    assert math.isfinite(path["spread_ms"]) and path["spread_ms"] >= 0


def test_bench_envmap_record():
    from taichi_gaussian_rasterizer_amd.benchmarks import bench_envmap
    args = bench_envmap.parse_args(["--envmap_size", "256,256", "--iters", "3", "--warmup", "1", "--n", "5000"])
    record = bench_envmap.bench_envmap(args)
    assert record["iters"] == 3 and record["rounds"] == 3 and len(record["cases"]) == 6
    assert [(case["edge"], case["weight"]) for case in record["cases"]] == \
        [(edge, kind) for edge in (64, 512) for kind in ("horizon", "sky", "noise")]
    for case in record["cases"]:
        assert (case["height"], case["width"], case["pixels"], case["channels"]) == (256, 256, 65536, 3)
        forward = 4 * (2 * 3 + 1) * 65536                               # image and weight read, image written
        backward = 4 * 3 * 65536 + 24 * case["edge"] ** 2 * 3          # gradient read, 6 R^2 C floats written
        for part, nbytes in (("forward", forward), ("forward_backward", forward + backward)):
            r = case[part]
            assert r["bytes"] == nbytes and isinstance(r["fused_faster"], bool)
            for path in ("fused", "torch", "stream"):
                _finite_path(r[path])
            for key in ("fused_tbps", "stream_tbps", "ratio_to_stream", "speedup"):
                assert math.isfinite(r[key]) and r[key] > 0, key
    t = record["training"]
    assert (t["height"], t["width"], t["n"], t["edge"]) == (256, 256, 5000, 512) and isinstance(t["fused_faster"], bool)
    for path in ("alone", "fused", "torch"):
        _finite_path(t[path])
    assert math.isfinite(t["added_ms"]) and math.isfinite(t["added_torch_ms"])
