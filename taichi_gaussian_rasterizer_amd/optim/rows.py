"""Row lists of a batch of views (csrc/rows.hip): the ascending runs of an index list, the sum of the runs' value rows
for the rows of a step, and the union of the views' visible sets with their summed visibility -- what one optimizer step
after several backward passes needs, without a sort.

    opt.zero_grad()
    rs = [render_gaussians(g, cam, cfg, use_sh=True, sparse_grad=True) for cam in cams]
    for r, target in zip(rs, targets): photometric_loss(r.image, target).backward()
    opt.step(*visible_union(rs))
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from .. import _native as nv

MAX_RUNS = 16  # GS_ROWS_MAX_RUNS (include/gsplat_hip.h)


def find_runs(rows: torch.Tensor, run_count: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(run_starts (MAX_RUNS + 1) int64, run_count (1) int32), both on the device: where the maximal strictly ascending
    runs of `rows` (int64, not empty) start.  No host read; `run_count`: a (1) int32 to write the count to."""
    nv.require_device(rows, dtype=torch.int64, what="row list")
    assert rows.dim() == 1 and rows.shape[0] > 0 and rows.is_contiguous(), "find_runs takes a contiguous, non-empty list"
    starts = torch.empty((MAX_RUNS + 1,), dtype=torch.int64, device=rows.device)
    if run_count is None:
        run_count = torch.empty((1,), dtype=torch.int32, device=rows.device)
    nv.check(nv.lib().gs_rows_find_runs(rows.shape[0], nv.ptr(rows), MAX_RUNS, nv.ptr(starts), nv.ptr(run_count),
                                        nv.stream()), "gs_rows_find_runs")
    return starts, run_count


def sum_runs(indexes: torch.Tensor, runs: int, run_starts: Optional[torch.Tensor], grad_indexes: torch.Tensor,
             grad_values: torch.Tensor) -> torch.Tensor:
    """(len(indexes), D) float32: for each row of `indexes` the sum, in run order, of the rows of `grad_values` (R, D)
    whose entry of `grad_indexes` (R, made of `runs` <= MAX_RUNS ascending runs) names it; zeros for a row none names"""
    nv.require_device(indexes, grad_indexes, run_starts, dtype=torch.int64, what="rows of a step")
    nv.require_device(grad_values, what="gradient rows")
    assert grad_values.dim() == 2 and grad_values.shape[0] == grad_indexes.shape[0], "one value row per listed row"
    indexes, grad_indexes, grad_values = indexes.contiguous(), grad_indexes.contiguous(), grad_values.contiguous()
    out = torch.empty((indexes.shape[0], grad_values.shape[1]), dtype=torch.float32, device=indexes.device)
    nv.check(nv.lib().gs_rows_sum_runs(indexes.shape[0], nv.ptr(indexes), int(runs), nv.ptr(run_starts),
                                       grad_indexes.shape[0], nv.ptr(grad_indexes), grad_values.shape[1],
                                       nv.ptr(grad_values), nv.ptr(out), nv.stream()), "gs_rows_sum_runs")
    return out


def _union_torch(cat: torch.Tensor, vcat: Optional[torch.Tensor], num_points: int):
    """the union by a sort: torch.unique, and index_add_ for the values (whose order of addition is index_add_'s)"""
    inside = (cat >= 0) & (cat < num_points)
    rows, inverse = torch.unique(cat[inside], return_inverse=True)
    if vcat is None:
        return rows, None
    return rows, torch.zeros(rows.shape[0], dtype=torch.float32, device=cat.device).index_add_(0, inverse, vcat[inside])


def union_rows(lists: Sequence[torch.Tensor], values: Optional[Sequence[torch.Tensor]] = None, *, num_points: int):
    """(rows, summed): `rows` = the ascending distinct int64 union of the row lists, entries outside [0, num_points)
    skipped (gs_rows_union: a bitmap over the rows, no sort); `summed[j]` = the sum over the lists, in list order, of
    values[b] at rows[j] (None without `values`).  Lists may be in any order and repeat rows; each list of a batch of
    views is ascending, so their concatenation has one run per view.  More than MAX_RUNS runs, or
    fractional.MERGE_RUNS = False: torch.unique and index_add_.  One host read (the size of the union and the number
    of runs, together)."""
    from . import fractional
    lists = list(lists)
    values = None if values is None else list(values)
    assert values is None or len(values) == len(lists), "one value tensor per list"
    for b, rows in enumerate(lists):
        assert rows.dim() == 1, "a row list is one-dimensional"
        assert values is None or values[b].shape == rows.shape, \
            f"list {b}: {tuple(values[b].shape)} values for {tuple(rows.shape)} rows"
    nv.require_device(*lists, dtype=torch.int64, what="union_rows lists")
    if values is not None:
        nv.require_device(*lists, *values, dtype=None, what="union_rows values")
        nv.require_device(*values, what="union_rows values")
    assert lists, "union_rows needs at least one list"
    device, n = lists[0].device, int(num_points)
    cat = (lists[0] if len(lists) == 1 else torch.cat(lists)).contiguous()
    vcat = None if values is None else (values[0] if len(values) == 1 else torch.cat(values)).contiguous()
    count = cat.shape[0]
    if count == 0 or n <= 0:
        return cat.new_empty((0,)), None if vcat is None else vcat.new_empty((0,))
    if not fractional.MERGE_RUNS:
        return _union_torch(cat, vcat, n)
    with torch.cuda.device(device):
        lib = nv.lib()
        need = lib.gs_rows_union_scratch_bytes(n)
        scratch = nv.scratch(need, device)
        union = torch.empty((min(count, n),), dtype=torch.int64, device=device)
        counts = torch.empty((2,), dtype=torch.int32, device=device)  # the union's size, the number of runs
        nv.check(lib.gs_rows_union(n, count, nv.ptr(cat), nv.ptr(union), nv.ptr(counts), nv.ptr(scratch), need,
                                   nv.stream()), "gs_rows_union")
        starts = None
        if vcat is not None:
            starts, _ = find_runs(cat, counts[1:])
        size, runs = counts.tolist() if vcat is not None else (int(counts[0]), 0)
        rows = union[:size]
        if vcat is None:
            return rows, None
        if runs > MAX_RUNS:
            return _union_torch(cat, vcat, n)
        return rows, sum_runs(rows, runs, starts, cat, vcat.unsqueeze(1)).squeeze(1)


def visible_union(renderings, *, num_points: Optional[int] = None):
    """(indexes, visibility) for `VisibilityAware*.step` after one backward per rendering: the union of the frames'
    `points_in_view` and the visibility summed over the views (a caller who wants the mean divides); visibility is None
    when the frames carry none.  `num_points`: the number of Gaussians; left out, it is taken from the largest row any
    frame lists, which costs a host read of its own.  A `RenderedViews` (render_views) carries the pair already: it is
    returned as stored, without a launch."""
    from ..renderer import RenderedViews
    if isinstance(renderings, RenderedViews):
        return renderings.points_in_view, renderings.point_visibility
    renderings = list(renderings)
    lists = [r.points_in_view for r in renderings]
    values = [r.point_visibility for r in renderings]
    if any(v is None for v in values):
        values = None
    else:
        values = [v.detach() for v in values]
    if num_points is None:
        last = [rows[-1:] for rows in lists if rows.shape[0] > 0]  # each list ascends
        num_points = int(torch.cat(last).max()) + 1 if last else 0
    return union_rows(lists, values, num_points=num_points)
