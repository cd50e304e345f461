"""Row-sparse optimizers driven by the renderer's visible set.

A training view touches only the Gaussians in `points_in_view`; these optimizers update exactly those rows, and
let a row take a *fraction* of a step (weight w in place of 1: moments decay by beta**w, the update is scaled by
1 - exp(-2 w)).  Semantics follow the reference (optim/fractional.py:17-222, optim/fractional_adam.py,
optim/fractional_laprop.py, optim/util.py): parameter groups hold ONE (N, ...) tensor each and are typed

    "scalar"        second moment per element
    "vector"        one second moment per row (norm of the row's gradient)
    "local_vector"  as "vector", in a per-row frame: `basis` (rows, D, D) maps local -> parameter coordinates

with optional `mask_lr` (per column) and `point_lr` (per row) multipliers.  The moment update -- and for the
first two group types the parameter update itself -- is one launch of gs_optim_step per group.

A parameter's `.grad` may be a `torch.sparse_coo` tensor over rows, as `render_gaussians(sparse_grad=True)` leaves
it: the step then reads the compact (V, D) values in place (gs_optim_step_rows); a row of `indexes` the gradient does
not list takes a zero gradient, as it would from the dense tensor.  A gradient that is one backward of one frame is
recognised by the address of its index list (fused.is_frame_sparse_grad) and trusted to be ascending: `indexes` is
matched against it by one binary-search launch, no host copy, no sort.  Any other sparse gradient -- summed over several
backward passes, built by hand, zero_grad(set_to_none=False) -- is seen as a concatenation of strictly ascending runs
(gs_rows_find_runs; the sum of B frame gradients has at most B, however autograd laid it out).  With at most
GS_ROWS_MAX_RUNS of them the gradient rows of the step's `indexes` are summed in run order (gs_rows_sum_runs: one
binary search per run, no sort) and the step reads those; this costs one 4-byte host read per step, the run counts of all
groups together.  With more runs, or with MERGE_RUNS = False, the gradient goes through `coalesce()` first: correct, but
slower.
"""
from __future__ import annotations

from functools import cached_property
from typing import Optional

import torch

from .. import _native as nv
from . import rows as row_lists

ADAM, LAPROP = 0, 1
_GROUP_TYPES = ("scalar", "vector", "local_vector")

# False: every sparse gradient that is neither a frame's own nor coalesced goes through coalesce(), and union_rows
# through torch.unique -- the path before the run kernels existed, for A/B runs
MERGE_RUNS = True


def saturate(x: torch.Tensor) -> torch.Tensor:
    """fraction of a full step a row with weight x takes: 1 - exp(-2 x)"""
    return -torch.expm1(-2.0 * x)


class _Rows:
    """One parameter group seen as an (N, D) matrix, with its optimizer state."""

    def __init__(self, group: dict, state: dict):
        tensors = group["params"]
        assert len(tensors) == 1, f"expected 1 tensor in group {group['name']}, got {len(tensors)}"
        (tensor,) = tensors
        self.tensor, self.state, self.options = tensor, state[tensor], group
        self.name, self.kind = group["name"], group["type"]
        if self.kind not in _GROUP_TYPES:
            raise ValueError(f"unknown group type {self.kind}")
        self.num_points = tensor.shape[0]
        self.param = tensor.view(self.num_points, -1)

    @cached_property
    def grad(self):
        """None, the (N, D) view of a dense gradient, or the _SparseRows of a sparse one -- formed on first use, since
        forming the latter may launch (find_runs) or sort (coalesce)"""
        grad = self.tensor.grad
        if grad is not None and grad.is_sparse:
            return _SparseRows(grad, self.param.shape[1])
        return None if grad is None else grad.view(self.num_points, -1)

    @property
    def per_row_moment(self) -> bool:
        return self.kind != "scalar"

    def moments(self):
        """(first moment (N, D), second moment (N, D) or (N)), created on first use.  Keys as in the reference's
        checkpoints (optim/util.py:5-18): first moment under 'v', second moment under 'm'."""
        st = self.state
        if "v" not in st:
            st["v"] = torch.zeros_like(self.param)
            st["m"] = self.param.new_zeros(self.num_points) if self.per_row_moment else torch.zeros_like(self.param)
        # a loaded state dict may hold non-contiguous moments: make the STATE contiguous once (the kernel updates the
        # buffers it is handed in place; a temporary copy would be updated and dropped, freezing the moments)
        for key in ("v", "m"):
            if not st[key].is_contiguous():
                st[key] = st[key].contiguous()
        return st["v"], st["m"]

    def shared(self, key: str) -> torch.Tensor:
        """an (N) float32 counter kept in this group's state (the first group carries the optimizer-wide ones)"""
        if key not in self.state:
            self.state[key] = torch.zeros(self.num_points, dtype=torch.float32, device=self.param.device)
        return self.state[key]


class _SparseRows:
    """A sparse row gradient seen as an ascending list of distinct rows (R) and their values (R, D) -- or, while
    `run_starts` is set, as up to GS_ROWS_MAX_RUNS such lists one behind the other (a sum over several backward
    passes), which `for_step` turns into the former for the rows of one step."""

    def __init__(self, grad: torch.Tensor, width: int):
        from ..fused import is_frame_sparse_grad
        if grad.sparse_dim() != 1:
            raise ValueError(f"a sparse gradient must be sparse over rows only, got sparse_dim {grad.sparse_dim()}")
        self.width, self.runs, self.run_starts, self.run_count = width, 0, None, None
        if grad.is_coalesced() or is_frame_sparse_grad(grad):
            self._adopt(grad)
        elif MERGE_RUNS and grad._nnz() > 0:
            self._adopt(grad)
            self.indexes = self.indexes.contiguous()
            self.run_starts, self.run_count = row_lists.find_runs(self.indexes)  # read on the host by settle_runs
            self._grad = grad
        else:
            self._adopt(grad.coalesce())  # the slow path: sorts, and sums repeated rows

    def _adopt(self, grad: torch.Tensor) -> None:
        self.indexes = grad._indices()[0]
        self.values = grad._values().reshape(self.indexes.shape[0], self.width)
        if not self.values.is_contiguous():
            self.values = self.values.contiguous()

    @staticmethod
    def settle_runs(grads) -> None:
        """the one host read of a step: the run counts of every gradient that waits for one.  A gradient of more than
        GS_ROWS_MAX_RUNS runs goes through coalesce() after all."""
        waiting = [g for g in grads if isinstance(g, _SparseRows) and g.run_count is not None]
        if not waiting:
            return
        counts = (waiting[0].run_count if len(waiting) == 1 else torch.cat([g.run_count for g in waiting])).tolist()
        for g, runs in zip(waiting, counts):
            g.run_count = None
            if runs <= row_lists.MAX_RUNS:
                g.runs = int(runs)
            else:
                g.run_starts = None
                g._adopt(g._grad.coalesce())
            g._grad = None

    def for_step(self, indexes: torch.Tensor) -> "_SparseRows":
        """the gradient as one list: itself, or -- made of runs -- the (len(indexes), D) rows of `indexes`, each the
        sum of its rows in the runs in run order, listed under `indexes` itself (rows_of: row i)"""
        assert self.run_count is None, "settle_runs first"
        if self.run_starts is None:
            return self
        summed = _SparseRows.__new__(_SparseRows)
        summed.width, summed.runs, summed.run_starts, summed.run_count = self.width, 0, None, None
        summed.indexes = indexes
        summed.values = row_lists.sum_runs(indexes, self.runs, self.run_starts, self.indexes, self.values)
        return summed

    def rows_of(self, indexes: torch.Tensor, cache: Optional[dict]):
        """int32 (len(indexes)): the row of `values` that holds the gradient of indexes[i], -1 for none; None when
        `indexes` IS the gradient's index list (row i)"""
        count = self.indexes.shape[0]
        if indexes.shape[0] == count and count > 0 and indexes.data_ptr() == self.indexes.data_ptr():
            return None
        key = (indexes.data_ptr(), indexes.shape[0], self.indexes.data_ptr(), count)
        found = None if cache is None else cache.get(key)
        if found is None:
            nv.require_device(indexes, self.indexes, dtype=torch.int64, what="optimizer step indexes")
            found = torch.empty((indexes.shape[0],), dtype=torch.int32, device=indexes.device)
            nv.check(nv.lib().gs_optim_grad_rows(indexes.shape[0], nv.ptr(indexes), count, nv.ptr(self.indexes),
                                                 nv.ptr(found), nv.stream()), "gs_optim_grad_rows")
            if cache is not None:
                cache[key] = found
        return found

    def gather(self, grad_rows: Optional[torch.Tensor], count: int) -> torch.Tensor:
        """(count, D) gradient rows in the order of `indexes`, zeros where the gradient has none"""
        if grad_rows is None:
            return self.values
        if self.values.shape[0] == 0:
            return self.values.new_zeros((count, self.values.shape[1]))
        at = grad_rows.to(torch.int64)
        return self.values[at.clamp_min(0)] * (at >= 0).unsqueeze(1)


@torch.no_grad()
def gather_sparse_grad(grad: torch.Tensor, indexes: torch.Tensor) -> torch.Tensor:
    """(len(indexes), D) float32: the rows `indexes` of a sparse row gradient (N, ...), D = the elements of a row, zeros
    where the gradient lists none; repeated rows of the gradient summed.  The three paths of the optimizer step: a frame's
    own or a coalesced gradient is read in place, a sum over up to GS_ROWS_MAX_RUNS backward passes run by run
    (in run order), anything else through coalesce()."""
    if not grad.is_sparse:
        raise TypeError("gather_sparse_grad takes a torch.sparse_coo gradient over rows")
    width = 1
    for extent in grad.shape[1:]:
        width *= int(extent)
    indexes = indexes.contiguous()
    nv.require_device(indexes, dtype=torch.int64, what="gather_sparse_grad indexes")
    nv.require_device(grad._values(), what="gather_sparse_grad values")
    rows = _SparseRows(grad, width)
    _SparseRows.settle_runs([rows])
    rows = rows.for_step(indexes)
    return rows.gather(rows.rows_of(indexes, None), indexes.shape[0])


def _launch(rows: _Rows, algorithm: int, indexes, weight, total_weight, grad, row_scale, in_place: bool,
            grad_rows=None, compact: bool = False):
    """gs_optim_step for one group; returns lr_step (rows, D) unless the update was applied in place.
    compact: `grad` is (R, D), visible row i reads its row grad_rows[i] (gs_optim_step_rows)"""
    m, v = rows.moments()
    opt = rows.options
    grad, indexes, weight = grad.contiguous(), indexes.contiguous(), weight.contiguous()
    scale = None if row_scale is None else row_scale.contiguous()
    # a state dict from elsewhere may hold anything under these keys: the kernel indexes m[idx * D + j] and
    # v[idx] / v[idx * D + j] without further checks
    second = (rows.num_points,) if rows.per_row_moment else tuple(rows.param.shape)
    if tuple(m.shape) != tuple(rows.param.shape):
        raise ValueError(f"{rows.name}: first moment (state['v']) has shape {tuple(m.shape)}, expected "
                         f"{tuple(rows.param.shape)}")
    if tuple(v.shape) != second:
        raise ValueError(f"{rows.name}: second moment (state['m']) has shape {tuple(v.shape)}, expected {second}")
    nv.require_device(grad, weight, m, v, total_weight, scale, what="optimizer step")
    nv.require_device(indexes, dtype=torch.int64, what="optimizer step indexes")
    count, width = indexes.shape[0], rows.param.shape[1]
    mask = per_point = None
    if in_place:
        if opt["mask_lr"] is not None:
            mask = opt["mask_lr"].reshape(-1).to(torch.float32).contiguous()
            assert mask.shape[0] == width, f"mask_lr has {mask.shape[0]} entries for {width} columns"
        if opt["point_lr"] is not None:
            per_point = opt["point_lr"].to(torch.float32).contiguous()
        nv.require_device(rows.param, mask, per_point, what="optimizer step")
    lr_step = None if in_place else rows.param.new_zeros(count, width)
    beta1, beta2 = opt["betas"]
    if compact:
        nv.require_device(grad_rows, dtype=torch.int32, what="optimizer step gradient rows")
        if grad.shape[0] > 0 and grad.shape[1] != width:
            raise ValueError(f"{rows.name}: gradient rows have {grad.shape[1]} columns, expected {width}")
        nv.check(nv.lib().gs_optim_step_rows(
            algorithm, int(rows.per_row_moment), count, width, nv.ptr(indexes), nv.ptr(weight), nv.ptr(m), nv.ptr(v),
            nv.ptr(total_weight), nv.ptr(grad) if grad.shape[0] > 0 else None, grad.shape[0], nv.ptr(grad_rows),
            float(opt["lr"]), float(beta1), float(beta2), float(opt["eps"]), int(opt["bias_correction"]),
            nv.ptr(lr_step), nv.ptr(scale), nv.ptr(rows.param) if in_place else None, nv.ptr(mask), nv.ptr(per_point),
            nv.stream()), "gs_optim_step_rows")
        return lr_step
    nv.check(nv.lib().gs_optim_step(algorithm, int(rows.per_row_moment), count, width, nv.ptr(indexes), nv.ptr(weight),
                                    nv.ptr(m), nv.ptr(v), nv.ptr(total_weight), nv.ptr(grad), float(opt["lr"]),
                                    float(beta1), float(beta2), float(opt["eps"]), int(opt["bias_correction"]),
                                    nv.ptr(lr_step), nv.ptr(scale), nv.ptr(rows.param) if in_place else None,
                                    nv.ptr(mask), nv.ptr(per_point), nv.stream()), "gs_optim_step")
    return lr_step


def update_rows(rows: _Rows, algorithm: int, indexes: torch.Tensor, weight: torch.Tensor, total_weight: torch.Tensor,
                basis: Optional[torch.Tensor] = None, row_scale: Optional[torch.Tensor] = None,
                cache: Optional[dict] = None) -> None:
    """One fractional step of the visible rows of one group (reference optim/fractional.py:107-147 + :57-63).
    `cache`: shared by the groups of one step, so that `indexes` is matched against a sparse gradient's rows once."""
    grad = rows.grad
    sparse = isinstance(grad, _SparseRows)
    extra = {}
    if sparse:
        indexes = indexes.contiguous()
        grad = grad.for_step(indexes)
        extra = dict(grad_rows=grad.rows_of(indexes, cache), compact=True)
    if rows.kind == "local_vector" and sparse:
        assert basis is not None, "basis is required for local_vector optimizer"
        # as below, on the compact rows: the local-frame gradient of the visible rows is (len(indexes), D) already
        visible = grad.gather(extra["grad_rows"], indexes.shape[0])
        if row_scale is not None:
            visible = visible * row_scale.unsqueeze(1)
        local = torch.einsum("bij,bj->bi", torch.linalg.inv(basis), visible)
        step = _launch(rows, algorithm, indexes, weight, total_weight, local, None, in_place=False, compact=True)
        step = torch.einsum("bij,bj->bi", basis, step)
        if rows.options["mask_lr"] is not None:
            step = step * rows.options["mask_lr"].reshape(1, -1)
        if rows.options["point_lr"] is not None:
            step = step * rows.options["point_lr"][indexes].unsqueeze(1)
        rows.param[indexes] -= step * saturate(weight).unsqueeze(1)
        return
    if sparse:
        grad = grad.values
    if rows.kind == "local_vector":
        assert basis is not None, "basis is required for local_vector optimizer"
        # gradient into the local frame, step back out of it; the kernel sees a scratch copy of the visible rows so
        # that the caller's .grad stays as autograd left it
        local = grad.clone()
        visible = grad[indexes] if row_scale is None else grad[indexes] * row_scale.unsqueeze(1)
        local[indexes] = torch.einsum("bij,bj->bi", torch.linalg.inv(basis), visible)
        step = _launch(rows, algorithm, indexes, weight, total_weight, local, None, in_place=False)
        step = torch.einsum("bij,bj->bi", basis, step)
        if rows.options["mask_lr"] is not None:
            step = step * rows.options["mask_lr"].reshape(1, -1)
        if rows.options["point_lr"] is not None:
            step = step * rows.options["point_lr"][indexes].unsqueeze(1)
        rows.param[indexes] -= step * saturate(weight).unsqueeze(1)
    elif rows.param.is_contiguous():
        _launch(rows, algorithm, indexes, weight, total_weight, grad, row_scale, in_place=True, **extra)
    else:  # a parameter that is a strided view: let torch do the scatter
        step = _launch(rows, algorithm, indexes, weight, total_weight, grad, row_scale, in_place=False, **extra)
        if rows.options["mask_lr"] is not None:
            step = step * rows.options["mask_lr"].reshape(1, -1)
        if rows.options["point_lr"] is not None:
            step = step * rows.options["point_lr"][indexes].unsqueeze(1)
        rows.param[indexes] -= step * saturate(weight).unsqueeze(1)


class FractionalOpt(torch.optim.Optimizer):
    """step(indexes, weight, basis=None): rows `indexes` take a step of fraction `weight` each"""
    algorithm = ADAM

    def __init__(self, param_groups: list, lr=0.001, betas=(0.9, 0.999), eps=1e-16, bias_correction=True, **extra):
        assert lr > 0, f"Invalid learning rate: {lr}"
        assert eps > 0, f"Invalid epsilon: {eps}"
        for i, beta in enumerate(betas, start=1):
            assert 0.0 <= beta < 1.0, f"Invalid beta{i}: {beta}"
        defaults = dict(lr=lr, betas=betas, eps=eps, mask_lr=None, point_lr=None, type="scalar",
                        bias_correction=bias_correction)
        defaults.update(extra)
        super().__init__(param_groups, defaults)

    def _rows(self):
        views = [_Rows(group, self.state) for group in self.param_groups]
        count = views[0].num_points
        for view in views:
            assert view.num_points == count, f"param shape {view.num_points} != {count}"
        return views

    @torch.no_grad()
    def _take_step(self, indexes, weight, basis=None, row_scale=None, counted: bool = False):
        """`counted`: total_weight already includes this step's weights"""
        assert weight.shape == indexes.shape, f"shape mismatch {weight.shape} != {indexes.shape}"
        views = self._rows()
        total_weight = views[0].shared("total_weight")
        if not counted:
            total_weight[indexes] += weight
        cache = {}
        _SparseRows.settle_runs([view.grad for view in views])
        for view in views:
            if view.grad is not None:
                update_rows(view, self.algorithm, indexes, weight, total_weight, basis, row_scale, cache)

    def step(self, indexes: torch.Tensor, weight: torch.Tensor, basis: Optional[torch.Tensor] = None):
        self._take_step(indexes, weight, basis)


class FractionalAdam(FractionalOpt):
    algorithm = ADAM


class FractionalLaProp(FractionalOpt):
    algorithm = LAPROP


class _WholeSteps(FractionalOpt):
    """step(indexes, basis=None): every listed row takes a full step (weight 1)"""

    def step(self, indexes: torch.Tensor, basis: Optional[torch.Tensor] = None):
        self._take_step(indexes, torch.ones(indexes.shape[0], device=indexes.device, dtype=torch.float32), basis)


class SparseAdam(_WholeSteps):
    algorithm = ADAM


class SparseLaProp(_WholeSteps):
    algorithm = LAPROP
