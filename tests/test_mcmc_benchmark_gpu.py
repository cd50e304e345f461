"""bench_mcmc runs (at a size that takes seconds) and its record has every figure it reports."""
import math

import pytest

pytestmark = pytest.mark.gpu


def timed(part, names):
    for name in names:
        assert len(part[name]["rounds"]) == 3
        assert math.isfinite(part[name]["ms"]) and part[name]["ms"] > 0 and part[name]["spread_ms"] >= 0


def test_bench_mcmc():
    from taichi_gaussian_rasterizer_amd.benchmarks import bench_mcmc
    n = 50000
    args = bench_mcmc.parse_args(["--n", str(n), "--degree", "1", "--iters", "3", "--rounds", "3", "--warmup", "1"])
    record = bench_mcmc.bench_mcmc(args)
    assert record["N"] == n and record["sh_degree"] == 1
    assert sorted(record["perturb"]) == ["mostly_closed", "open", "scene"]
    for case, part in record["perturb"].items():
        timed(part, ("torch", "perturb"))
        assert isinstance(part["perturb_faster"], bool)
        for kernel in (part["kernel"], part["kernel_cold"]):
            assert kernel["calls"] == 9 and kernel["ms"] > 0 and kernel["tbps"] > 0 and kernel["move_tbps"] > 0
            assert 0 <= kernel["open_rows"] <= n and 0 <= kernel["changed_components"] <= 3 * kernel["open_rows"]
            assert kernel["bytes"] == 4 * n + 52 * kernel["open_rows"] + 4 * kernel["changed_components"]
    closed, opened = record["perturb"]["mostly_closed"]["kernel"], record["perturb"]["open"]["kernel"]
    assert opened["open_rows"] == n and 0.15 * n < closed["open_rows"] < 0.3 * n
    assert opened["bytes_per_row"] > 56 and closed["bytes_per_row"] < 24
    timed(record["relocate"], ("composition", "relocate"))
    timed(record["grow"], ("composition", "grow"))
    assert isinstance(record["relocate"]["relocate_faster"], bool) and isinstance(record["grow"]["grow_faster"], bool)
    assert 0 < record["relocate"]["dead_rows"] < n // 10 and record["grow"]["new_rows"] == n // 20
    assert record["relocate"]["tables"] >= 10
