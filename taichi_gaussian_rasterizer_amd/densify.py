"""Densification on the device: prune, clone and split the rows of a scene together with their optimizer state.

    stats = DensifyStats(n, device)                    # once per densification interval
    stats.update(rendering)                            # after each backward: one launch
    plan = plan_densify(prune=..., split=..., clone=..., children=2)     # the ONE read-back: the four counts
    params = densify(params, plan)                     # one move launch for every column and state table, one split

`plan_densify` turns three boolean masks into `src_of`, the source row of every output row, in a fixed order: the
kept rows ascending (exactly `(~(prune | split)).nonzero()`), then the clones ascending by parent, then the children
of the split rows, parent-major.  Per row prune wins over split and split over clone.  `densify` and `move_rows` move
tables by that plan with gs_table_move_rows; `split_gaussians3d` and `densify` place the children with
gs_split3d_children.  Choosing the rows (thresholds, top-k) stays in torch.  Everything here runs on a HIP device only.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _native as nv
from .data_types import Gaussians3D
from .optim.parameter_class import ParameterClass, TensorTable

_STATE_MODES = ("zero", "parent")
_SPLIT_COLUMNS = ("position", "log_scaling", "rotation")


@dataclasses.dataclass(frozen=True)
class DensifyPlan:
    """`src_of` (rows,) int32: the source row of every output row; the counts as Python ints.
    rows = kept + clones + children * split_parents; `num_source` is the number of rows the masks had."""
    src_of: torch.Tensor
    kept: int
    clones: int
    split_parents: int
    rows: int
    children: int
    num_source: int

    @property
    def num_children(self) -> int:
        return self.children * self.split_parents

    @property
    def first_child(self) -> int:
        """output row of the first child"""
        return self.kept + self.clones


def _check_mask(name: str, mask, rows: Optional[int]) -> int:
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"plan_densify: {name} must be a torch.Tensor, got {type(mask).__name__}")
    if mask.dtype != torch.bool:
        raise TypeError(f"plan_densify: {name} must be a bool mask, got {mask.dtype}")
    if mask.dim() != 1 or (rows is not None and int(mask.shape[0]) != rows):
        want = "(N,)" if rows is None else f"({rows},)"
        raise ValueError(f"plan_densify: {name} has shape {tuple(mask.shape)}, expected {want}")
    return int(mask.shape[0])


def plan_densify(prune: Optional[torch.Tensor] = None, split: Optional[torch.Tensor] = None,
                 clone: Optional[torch.Tensor] = None, *, children: int = 2,
                 max_rows: Optional[int] = None) -> DensifyPlan:
    """Masks -> DensifyPlan.  prune, split, clone: bool (N,) on the device, None = no row; at least one is given.
    Reads the four counts back once (the only synchronisation of a densification, like the tile mapper's K).
    max_rows: the most rows the result may have; ValueError when the plan needs more (the capacity of `src_of` is
    max_rows, or N * max(2, children) without it, which always suffices)."""
    masks = dict(prune=prune, split=split, clone=clone)
    n = None
    for name, mask in masks.items():
        if mask is not None:
            n = _check_mask(name, mask, n)
    if n is None:
        raise ValueError("plan_densify: no mask given (the number of rows comes from the masks)")
    children = int(children)
    if not 1 <= children <= nv.GS_DENSIFY_CHILDREN_MAX:
        raise ValueError(f"plan_densify: children {children} not in [1, {nv.GS_DENSIFY_CHILDREN_MAX}]")
    if max_rows is not None and int(max_rows) < 0:
        raise ValueError(f"plan_densify: max_rows {max_rows}")
    if n * max(2, children) >= 2 ** 31:
        raise ValueError(f"plan_densify: {n} rows with {children} children (N * max(2, children) must stay below 2^31)")
    given = [m for m in masks.values() if m is not None]
    nv.require_device(*given, dtype=None, what="plan_densify")
    device = given[0].device
    capacity = n * max(2, children) if max_rows is None else int(max_rows)
    if n == 0:
        return DensifyPlan(torch.empty((0,), dtype=torch.int32, device=device), 0, 0, 0, 0, children, 0)
    prune, split, clone = (None if m is None else m.contiguous() for m in masks.values())
    with torch.cuda.device(device):
        lib = nv.lib()
        src_of = torch.empty((capacity,), dtype=torch.int32, device=device)
        counts = torch.empty((4,), dtype=torch.int32, device=device)
        need = lib.gs_densify_plan_scratch_bytes(n)
        scratch = nv.scratch(need, device)
        nv.check(lib.gs_densify_plan(n, nv.ptr(prune), nv.ptr(split), nv.ptr(clone), children, capacity,
                                     nv.ptr(src_of), nv.ptr(counts), nv.ptr(scratch), need, nv.stream()),
                 "gs_densify_plan")
        kept, clones, parents, rows = (int(c) for c in counts.tolist())
    if rows > capacity:
        raise ValueError(f"plan_densify: the plan has {rows} rows ({kept} kept, {clones} clones, {parents} split into "
                         f"{children}), max_rows is {capacity}")
    return DensifyPlan(src_of[:rows], kept, clones, parents, rows, children, n)


def _kernel_moves(t: torch.Tensor) -> bool:
    """does gs_table_move_rows take this column?  Contiguous rows of a multiple of 4 bytes."""
    row_bytes = t[0].numel() * t.element_size() if t.shape[0] > 0 else 0
    return t.is_contiguous() and row_bytes > 0 and row_bytes % 4 == 0 and t.data_ptr() % 4 == 0


def _move(columns: Sequence[Tuple[torch.Tensor, int]], plan: DensifyPlan, what: str) -> List[torch.Tensor]:
    """[(column, copy_rows)] -> the moved columns: new[j] = column[src_of[j]] for j < copy_rows, zero behind"""
    columns = [(t.detach(), int(c)) for t, c in columns]
    for t, c in columns:
        if t.dim() < 1 or int(t.shape[0]) != plan.num_source:
            raise ValueError(f"{what}: a column has shape {tuple(t.shape)}, the plan was made for {plan.num_source} rows")
        if not 0 <= c <= plan.rows:
            raise ValueError(f"{what}: copy_rows {c} outside [0, {plan.rows}]")
    nv.require_device(plan.src_of, *(t for t, _ in columns), dtype=None, what=what)
    rows = plan.rows
    out: List[torch.Tensor] = []
    batch: List[nv.GsMoveColumn] = []
    if not columns:
        return out

    def flush():
        if batch:
            arr = (nv.GsMoveColumn * len(batch))(*batch)
            nv.check(nv.lib().gs_table_move_rows(rows, nv.ptr(plan.src_of), len(batch), arr, nv.stream()),
                     "gs_table_move_rows")
            batch.clear()

    with torch.cuda.device(plan.src_of.device):
        for t, copy_rows in columns:
            if rows == 0 or not _kernel_moves(t):
                new = t[plan.src_of.long()] if rows > 0 else t.new_empty((0, *t.shape[1:]))
                if copy_rows < rows:
                    new[copy_rows:] = 0
                out.append(new)
                continue
            new = torch.empty((rows, *t.shape[1:]), dtype=t.dtype, device=t.device)
            batch.append(nv.GsMoveColumn(t.data_ptr(), new.data_ptr(), t[0].numel() * t.element_size(), copy_rows))
            out.append(new)
            if len(batch) == nv.GS_MOVE_COLUMNS_MAX:
                flush()
        flush()
    return out


def move_rows(table, plan: DensifyPlan, copy_rows: Optional[int] = None) -> TensorTable:
    """The plan applied to any name -> tensor mapping with N rows (a TensorTable, dict(Gaussians3D.items()), a user's
    own per-Gaussian buffers): new[name][j] = table[name][plan.src_of[j]] for j < copy_rows (default: every row), zero
    from copy_rows on.  All columns go through gs_table_move_rows, GS_MOVE_COLUMNS_MAX (32) per launch; a column that
    is not contiguous or whose rows are not a multiple of 4 bytes (a bool column) is indexed in torch instead."""
    items = list(table.items() if hasattr(table, "items") else table)
    copy_rows = plan.rows if copy_rows is None else int(copy_rows)
    moved = _move([(t, copy_rows) for _, t in items], plan, "move_rows")
    return TensorTable({name: new for (name, _), new in zip(items, moved)})


def _check_noise(noise, shape, what: str):
    if noise is None:
        return
    if not isinstance(noise, torch.Tensor) or tuple(noise.shape) != tuple(shape):
        got = tuple(noise.shape) if isinstance(noise, torch.Tensor) else type(noise).__name__
        raise ValueError(f"{what}: noise has shape {got}, expected {tuple(shape)}")
    if noise.dtype != torch.float32:
        raise TypeError(f"{what}: noise must be float32, got {noise.dtype}")


def _log_shrink(shrink: float, what: str) -> float:
    if not float(shrink) > 0:
        raise ValueError(f"{what}: shrink {shrink} must be positive")
    return math.log(float(shrink))


def _split_children(count: int, children: int, parent_of: torch.Tensor, source: Dict[str, torch.Tensor],
                    noise: torch.Tensor, log_shrink: float, child_position: torch.Tensor,
                    child_log_scaling: torch.Tensor) -> None:
    position, log_scaling, rotation = (source[name].detach().contiguous() for name in _SPLIT_COLUMNS)
    noise = noise.contiguous()
    nv.require_device(position, log_scaling, rotation, noise, child_position, child_log_scaling,
                      what="gs_split3d_children")
    assert child_position.is_contiguous() and child_log_scaling.is_contiguous() and parent_of.is_contiguous()
    with torch.cuda.device(position.device):
        nv.check(nv.lib().gs_split3d_children(count, children, nv.ptr(parent_of), nv.ptr(position), nv.ptr(log_scaling),
                                              nv.ptr(rotation), nv.ptr(noise), log_shrink, nv.ptr(child_position),
                                              nv.ptr(child_log_scaling), nv.stream()), "gs_split3d_children")


def densify(params: ParameterClass, plan: DensifyPlan, *, noise: Optional[torch.Tensor] = None, shrink: float = 1.6,
            state: str = "zero") -> ParameterClass:
    """A new ParameterClass with the plan's rows: what `params[keep]` followed by `append_tensors(clones and
    children)` builds, in one move launch per 32 tables.

    Every column of `params.tensors` and every per-row entry of `params.tensor_state` goes through
    gs_table_move_rows.  Parameter columns copy all rows (a clone and a child start as their parent).  State columns
    copy the kept rows and start the new rows at zero with state="zero", as append_tensors does, or copy the parent's
    state into the new rows with state="parent".  `other_state` (step counts) and the parameter groups carry over.
    A column that is not contiguous or whose rows are not a multiple of 4 bytes (a bool column) is indexed in torch
    (`t[src_of]`, its tail zero-filled where that applies) instead of by the kernel.

    With split rows in the plan the table must have position, log_scaling and rotation (float32); their children get
    position = parent + R(rotation) (exp(log_scaling) * noise) and log_scaling = parent - log(shrink)
    (gs_split3d_children); rotation, opacity and features stay the parent's.  noise: (children * split_parents, 3)
    float32, child-major as the plan lists the children; default torch.randn on the device.

    No host synchronisation (the plan already has the counts).  CPU tensors raise; there is no CPU path."""
    what = "densify"
    if state not in _STATE_MODES:
        raise ValueError(f"{what}: state must be one of {_STATE_MODES}, got {state!r}")
    tensors = params.tensors
    count = plan.num_children
    if count > 0:
        missing = [name for name in _SPLIT_COLUMNS if name not in tensors]
        if missing:
            raise ValueError(f"{what}: the plan splits {plan.split_parents} rows, which needs the columns "
                             f"{list(_SPLIT_COLUMNS)}; the table has no {missing}")
    _check_noise(noise, (count, 3), what)
    log_shrink = _log_shrink(shrink, what)
    per_row = params.tensor_state
    state_rows = plan.kept if state == "zero" else plan.rows
    names = list(tensors.keys())
    state_keys = [(name, key) for name, table in per_row.items() for key in table.keys()]
    columns = [(tensors[name], plan.rows) for name in names] + [(per_row[n][k], state_rows) for n, k in state_keys]
    moved = _move(columns, plan, what)
    new_tensors = dict(zip(names, moved[:len(names)]))
    new_state: Dict[str, dict] = {name: {} for name in per_row}
    for (name, key), t in zip(state_keys, moved[len(names):]):
        new_state[name][key] = t
    if count > 0:
        if noise is None:
            noise = torch.randn((count, 3), dtype=torch.float32, device=plan.src_of.device)
        first = plan.first_child
        _split_children(count, plan.children, plan.src_of[first:], tensors, noise, log_shrink,
                        new_tensors["position"][first:], new_tensors["log_scaling"][first:])
    return params._rebuilt(TensorTable(new_tensors), {name: TensorTable(t) for name, t in new_state.items()})


def split_gaussians3d(gaussians: Gaussians3D, noise: torch.Tensor, shrink: float = 1.6) -> Gaussians3D:
    """Every row split into noise.shape[1] children (noise: (N, children, 3) float32), parent-major: rows
    [i * children, (i + 1) * children) are the children of row i.  Position and log_scaling as `densify` gives a split
    row's children; rotation, alpha_logit and feature are the parent's."""
    what = "split_gaussians3d"
    n = int(gaussians.batch_size[0])
    if not isinstance(noise, torch.Tensor) or noise.dim() != 3 or noise.shape[0] != n or noise.shape[2] != 3:
        got = tuple(noise.shape) if isinstance(noise, torch.Tensor) else type(noise).__name__
        raise ValueError(f"{what}: noise has shape {got}, expected ({n}, children, 3)")
    children = int(noise.shape[1])
    if not 1 <= children <= nv.GS_DENSIFY_CHILDREN_MAX:
        raise ValueError(f"{what}: {children} children per row, not in [1, {nv.GS_DENSIFY_CHILDREN_MAX}]")
    _check_noise(noise, (n, children, 3), what)
    log_shrink = _log_shrink(shrink, what)
    source = dict(gaussians.items())
    nv.require_device(*(source[name] for name in _SPLIT_COLUMNS), noise, what=what)
    device = gaussians.position.device
    src_of = torch.arange(n, dtype=torch.int32, device=device).repeat_interleave(children)
    plan = DensifyPlan(src_of, 0, 0, n, n * children, children, n)
    moved = move_rows(source, plan)
    if n > 0:
        _split_children(n * children, children, src_of, source, noise.reshape(n * children, 3), log_shrink,
                        moved["position"], moved["log_scaling"])
    return Gaussians3D(**moved, batch_size=(n * children,))


class DensifyStats:
    """Per-Gaussian densification signals summed over views: a float32 (num_points, 6) table on the device,
    `update`d by one launch per view (gs_densify_accumulate) and read through the column views

        seen            views in which the row was visible (visibility > 0; every listed row without visibility)
        viewspace_grad  sum of |dL/d(projected mean)|, the classic densification signal
        prune_cost, split_score   sums of Rendering.point_heuristic's columns
        visibility      sum of Rendering.point_visibility
        max_radius      largest projected sigma seen

    A table belongs to one row count: after `densify`, make a new one of the new size."""

    COLUMNS = ("seen", "viewspace_grad", "prune_cost", "split_score", "visibility", "max_radius")

    def __init__(self, num_points: int, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"DensifyStats: got device {device}; taichi_gaussian_rasterizer_amd runs on a HIP device "
                               "only")
        self.num_points = int(num_points)
        self.stats = torch.zeros((self.num_points, nv.GS_DENSIFY_STATS), dtype=torch.float32, device=device)

    def reset(self) -> "DensifyStats":
        self.stats.zero_()
        return self

    def update(self, rendering) -> "DensifyStats":
        """Add one view (a Rendering) or a batch of them (RenderedViews, any sequence of Renderings), after the
        backward pass: reads points_in_view, gaussians2d and its .grad where there is one (`gaussians2d.retain_grad()`
        before the backward), point_heuristic and point_visibility where the config produced them."""
        if not hasattr(rendering, "gaussians2d"):
            for view in rendering:
                self.update(view)
            return self
        g2d = rendering.gaussians2d
        grad = g2d.grad if (g2d.is_leaf or g2d.retains_grad) else None
        return self.update_rows(rendering.points_in_view, grad2d=grad, heuristic=rendering.point_heuristic,
                                visibility=rendering.point_visibility, gaussians2d=g2d)

    def update_rows(self, points_in_view: torch.Tensor, grad2d: Optional[torch.Tensor] = None,
                    heuristic: Optional[torch.Tensor] = None, visibility: Optional[torch.Tensor] = None,
                    gaussians2d: Optional[torch.Tensor] = None) -> "DensifyStats":
        """The same from explicit tensors: points_in_view (V,) int64, distinct rows (a repeated row gives undefined
        sums); grad2d (V, >= 2), the mean's gradient in its first two columns; heuristic (V, 2); visibility (V,);
        gaussians2d (V, 7).  None leaves the columns of that input untouched."""
        what = "DensifyStats.update_rows"
        v = int(points_in_view.shape[0])
        if points_in_view.dim() != 1 or points_in_view.dtype != torch.int64:
            raise TypeError(f"{what}: points_in_view must be (V,) int64, got {tuple(points_in_view.shape)} "
                            f"{points_in_view.dtype}")
        for name, t, ok in (("grad2d", grad2d, lambda t: t.dim() == 2 and t.shape[1] >= 2),
                            ("heuristic", heuristic, lambda t: t.dim() == 2 and t.shape[1] == 2),
                            ("visibility", visibility, lambda t: t.dim() == 1),
                            ("gaussians2d", gaussians2d, lambda t: t.dim() == 2 and t.shape[1] == 7)):
            if t is not None and (t.shape[0] != v or not ok(t)):
                raise ValueError(f"{what}: {name} has shape {tuple(t.shape)} for {v} listed rows")
        nv.require_device(self.stats, grad2d, heuristic, visibility, gaussians2d, what=what)
        nv.require_device(points_in_view, dtype=None, what=what)
        nv.check_same_device((self.stats, points_in_view))
        if v == 0 or self.num_points == 0:
            return self
        stride = 0
        if grad2d is not None:
            grad2d = grad2d.detach()
            if grad2d.stride(1) != 1 or grad2d.stride(0) < 2:
                grad2d = grad2d.contiguous()
            stride = int(grad2d.stride(0))
        heuristic, visibility, gaussians2d = (None if t is None else t.detach().contiguous()
                                              for t in (heuristic, visibility, gaussians2d))
        points_in_view = points_in_view.contiguous()
        with torch.cuda.device(self.stats.device):
            nv.check(nv.lib().gs_densify_accumulate(self.num_points, v, nv.ptr(points_in_view), nv.ptr(grad2d), stride,
                                                    nv.ptr(heuristic), nv.ptr(visibility), nv.ptr(gaussians2d),
                                                    nv.ptr(self.stats), nv.stream()), "gs_densify_accumulate")
        return self

    seen = property(lambda self: self.stats[:, 0])
    viewspace_grad = property(lambda self: self.stats[:, 1])
    prune_cost = property(lambda self: self.stats[:, 2])
    split_score = property(lambda self: self.stats[:, 3])
    visibility = property(lambda self: self.stats[:, 4])
    max_radius = property(lambda self: self.stats[:, 5])

    @property
    def mean_viewspace_grad(self) -> torch.Tensor:
        """viewspace_grad per view in which the row was seen (0 for rows never seen)"""
        return self.viewspace_grad / self.seen.clamp(min=1.0)


__all__ = ["DensifyPlan", "DensifyStats", "densify", "move_rows", "plan_densify", "split_gaussians3d"]
