"""bench_densify runs (at a size that takes seconds) and its record has every figure it reports."""
import math

import pytest

pytestmark = pytest.mark.gpu


def test_bench_densify():
    from taichi_gaussian_rasterizer_amd.benchmarks import bench_densify
    args = bench_densify.parse_args(["--n", "50000", "--degree", "1", "--iters", "3", "--rounds", "3", "--warmup", "1"])
    record = bench_densify.bench_densify(args)
    surgery, stats = record["surgery"], record["stats"]
    for part, names in ((surgery, ("composition", "densify", "densify_planned")), (stats, ("index_add", "update_rows"))):
        for name in names:
            assert len(part[name]["rounds"]) == 3
            assert math.isfinite(part[name]["ms"]) and part[name]["ms"] > 0 and part[name]["spread_ms"] >= 0
    plan = surgery["plan"]
    assert plan["rows"] == plan["kept"] + plan["clones"] + 2 * plan["split_parents"]
    assert 0 < plan["split_parents"] < 50000 and 0 < plan["clones"] < 50000
    move = surgery["move"]
    assert move["calls"] == 9 and move["ms"] > 0 and move["tbps"] > 0 and move["bytes"] > 50000 * 92
    assert isinstance(surgery["densify_faster"], bool) and isinstance(stats["update_faster"], bool)
