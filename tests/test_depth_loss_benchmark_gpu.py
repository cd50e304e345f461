"""benchmarks/bench_depth_loss.py at 256 x 256 with 3 iterations: the record holds every figure, the figures are finite,
and the byte counts are the stated per-pixel formulas."""
import math

import pytest

pytestmark = pytest.mark.gpu


def _finite_path(path):
    assert len(path["rounds"]) == 3
    assert all(math.isfinite(v) and v > 0 for v in path["rounds"] + [path["ms"]])
    assert math.isfinite(path["spread_ms"]) and path["spread_ms"] >= 0


def test_bench_depth_loss_record():
    from taichi_gaussian_rasterizer_amd.benchmarks import bench_depth_loss
    args = bench_depth_loss.parse_args(["--depth_size", "256,256", "--iters", "3", "--warmup", "1", "--n", "5000"])
    record = bench_depth_loss.bench_depth_loss(args)
    assert record["iters"] == 3 and record["rounds"] == 3 and len(record["cases"]) == 4
    assert [(case["masked"], case["loss"]) for case in record["cases"]] == \
        [(masked, loss) for masked in (False, True) for loss in ("affine", "pearson")]
    for case in record["cases"]:
        assert (case["height"], case["width"], case["pixels"]) == (256, 256, 65536)
        sweep = (12 if case["masked"] else 8) * 65536              # depth and prior, and the mask, read once
        forward = (2 if case["loss"] == "affine" else 1) * sweep   # moments, then residuals; Pearson: moments alone
        backward = sweep + 4 * 65536                               # read once more, the gradient written
        for part, nbytes in (("forward", forward), ("forward_backward", forward + backward)):
            r = case[part]
            assert r["bytes"] == nbytes and isinstance(r["fused_faster"], bool)
            for path in ("fused", "torch", "stream"):
                _finite_path(r[path])
            for key in ("fused_tbps", "stream_tbps", "ratio_to_stream", "speedup"):
                assert math.isfinite(r[key]) and r[key] > 0, key
    t = record["training"]
    assert (t["height"], t["width"], t["n"]) == (256, 256, 5000) and isinstance(t["fused_faster"], bool)
    for path in ("alone", "fused", "torch"):
        _finite_path(t[path])
    assert math.isfinite(t["added_ms"]) and math.isfinite(t["added_torch_ms"])
