"""Steps over a batch of views, the part that needs no GPU: the row-list entry points (gs_rows_find_runs,
gs_rows_sum_runs, gs_rows_union) validate their arguments on the host before any launch, an empty call is a no-op, and
the public helpers and the MERGE_RUNS switch exist and check their arguments before anything is launched."""
import ctypes
import os

import pytest
import torch

from taichi_gaussian_rasterizer_amd import _native

P = ctypes.c_void_p(16)  # a non-NULL pointer that is never dereferenced: every call below stops at a host-side check
MAX_RUNS = 16


def _err(lib):
    return lib.gs_last_error()


def test_find_runs_validates_on_the_host():
    lib = _native.lib()

    def call(count, rows=P, max_runs=MAX_RUNS, starts=P, run_count=P):
        return lib.gs_rows_find_runs(count, rows, max_runs, starts, run_count, None)

    assert call(10, rows=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(10, starts=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(10, run_count=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(-1) == -1 and b"count" in _err(lib)
    for bad in (0, -1, MAX_RUNS + 1):
        assert call(10, max_runs=bad) == -1 and b"max_runs" in _err(lib), bad
    assert call(0, max_runs=0) == -1          # the range holds for an empty list too
    assert call(0, rows=None, starts=None, run_count=None) == 0
    assert call(0, max_runs=1) == 0


def test_sum_runs_validates_on_the_host():
    lib = _native.lib()

    def call(rows, indexes=P, runs=2, starts=P, grad_count=10, grad_indexes=P, dims=3, values=P, out=P):
        return lib.gs_rows_sum_runs(rows, indexes, runs, starts, grad_count, grad_indexes, dims, values, out, None)

    assert call(10, indexes=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(10, out=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(10, starts=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(10, grad_indexes=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(10, values=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(-1) == -1 and b"rows" in _err(lib)
    assert call(10, grad_count=-1) == -1 and b"rows" in _err(lib)
    for dims in (0, -3):
        assert call(10, dims=dims) == -1 and b"dims" in _err(lib), dims
    for runs in (-1, MAX_RUNS + 1):
        assert call(10, runs=runs) == -1 and b"runs" in _err(lib), runs
    assert call(0, dims=0) == -1              # the ranges hold for an empty call too
    assert call(0, indexes=None, starts=None, grad_indexes=None, values=None, out=None) == 0
    assert call(0, runs=MAX_RUNS) == 0


def test_union_validates_on_the_host():
    lib = _native.lib()
    n = 100_000
    need = lib.gs_rows_union_scratch_bytes(n)

    def call(n_, count, rows=P, union=P, union_count=P, scratch=P, scratch_bytes=need):
        return lib.gs_rows_union(n_, count, rows, union, union_count, scratch, scratch_bytes, None)

    assert call(n, 10, rows=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(n, 10, union=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(n, 10, union_count=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(n, -1) == -1 and b"entries" in _err(lib)
    assert call(-1, 10) == -1 and b"entries" in _err(lib)
    assert call(n, 10, scratch_bytes=need - 1) == -4 and b"scratch" in _err(lib)
    assert call(n, 10, scratch=None) == -4 and b"scratch" in _err(lib)
    assert call(n, 10, scratch=ctypes.c_void_p(8)) == -1 and b"aligned" in _err(lib)
    assert call(n, 0, rows=None, union=None, union_count=None, scratch=None, scratch_bytes=0) == 0
    assert call(0, 10, rows=None, union=None, union_count=None, scratch=None, scratch_bytes=0) == 0
    for size in (1, 31, 32, 33, 1000, n, 32768, 32769, 4_000_000):
        assert lib.gs_rows_union_scratch_bytes(size) >= (size + 7) // 8, size
    assert lib.gs_rows_union_scratch_bytes(0) == 0


def test_helpers_and_switch_are_public():
    from taichi_gaussian_rasterizer_amd import optim
    from taichi_gaussian_rasterizer_amd.optim import fractional, rows
    for name in ("gather_sparse_grad", "union_rows", "visible_union"):
        assert name in optim.__all__ and callable(getattr(optim, name)), name
    assert fractional.MERGE_RUNS is True
    assert rows.MAX_RUNS == MAX_RUNS
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "gsplat_hip.h")).read()
    assert f"#define GS_ROWS_MAX_RUNS {MAX_RUNS}\n" in header


def test_union_rows_checks_its_arguments_before_any_launch():
    """one value tensor per list and one value per row (AssertionError); a tensor that is not on the HIP device, or of
    the wrong type, is refused by _native.require_device -- on CPU tensors it is the device it names"""
    from taichi_gaussian_rasterizer_amd.optim import union_rows
    a, b = torch.tensor([1, 4, 7]), torch.tensor([2, 4])
    with pytest.raises(AssertionError):
        union_rows([a, b], [torch.ones(3)], num_points=10)
    with pytest.raises(AssertionError):
        union_rows([a, b], [torch.ones(3), torch.ones(3)], num_points=10)
    with pytest.raises(RuntimeError, match="HIP device only"):
        union_rows([a, b], num_points=10)
    with pytest.raises(RuntimeError, match="HIP device only"):
        union_rows([a.to(torch.int32)], num_points=10)
