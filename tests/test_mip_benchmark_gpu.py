"""bench_mip runs (at a size that takes seconds) and its record has every figure it reports."""
import math

import pytest

pytestmark = pytest.mark.gpu


def timed(part, names):
    for name in names:
        assert len(part[name]["rounds"]) == 3
        assert math.isfinite(part[name]["ms"]) and part[name]["ms"] > 0 and part[name]["spread_ms"] >= 0


def test_bench_mip():
    from taichi_gaussian_rasterizer_amd.benchmarks import bench_mip
    n, cameras = 5000, 8
    args = bench_mip.parse_args(["--n", str(n), "--cameras", str(cameras), "--image_size", "256,256", "--degree", "1",
                                 "--iters", "3", "--rounds", "3", "--warmup", "1"])
    record = bench_mip.bench_mip(args)
    assert record["N"] == n and record["sh_degree"] == 1 and record["image_size"] == [256, 256]
    rate = record["sampling_rate"]
    timed(rate, ("torch", "sampling_rate"))
    assert isinstance(rate["sampling_rate_faster"], bool) and rate["seen_equal_torch"] in (True, False)
    kernel = rate["kernel"]
    assert kernel["calls"] == 9 and kernel["ms"] > 0 and kernel["pairs"] == n * cameras
    assert math.isfinite(kernel["pairs_per_second"]) and kernel["pairs_per_second"] > 0
    assert 0 < kernel["valu_share"] < 1 and kernel["valu_per_pair"] == bench_mip.VALU_PER_PAIR
    assert 0 < rate["seen_rows"] <= n and 0 < kernel["valid_pairs"] <= n * cameras
    assert rate["mean_cameras_per_seen_row"] >= 1
    smooth = record["smooth3d"]
    timed(smooth, ("torch_forward", "forward", "torch_forward_backward", "forward_backward", "forward_backward_rows"))
    assert smooth["N"] == n and 0 < smooth["V"] <= n
    for name, rows, per_row in (("gs_smooth3d_fwd", n, 36), ("gs_smooth3d_bwd", n, 52),
                                ("gs_smooth3d_bwd_rows", smooth["V"], 60)):
        for key in ("kernel", "kernel_cold"):
            k = smooth[f"{name}_{key}"]
            assert k["calls"] == 9 and k["ms"] > 0 and k["rows"] == rows and k["bytes"] == rows * per_row
            assert math.isfinite(k["tbps"]) and k["tbps"] > 0 and k["perturb_tbps"] > 0 and k["move_tbps"] > 0
    iteration = record["iteration"]
    timed(iteration, ("smooth3d", "none", "torch"))
    assert 0 < iteration["visible"] <= n  # of the smoothed set: larger splats, a few more pass the cull
    assert iteration["log_scaling_grad_sparse"]["smooth3d"] is True and iteration["log_scaling_grad_sparse"]["none"] is True
    assert iteration["log_scaling_grad_sparse"]["torch"] is False  # the composition's gradients arrive dense
    assert math.isfinite(iteration["smooth3d_cost_ms"]) and math.isfinite(iteration["torch_cost_ms"])
