"""The fixed-budget MCMC strategy ("3D Gaussian Splatting as Markov Chain Monte Carlo") on the device.

    perturb(params, lr)                                   # every iteration: opacity-gated noise on the positions
    relocate(params, dead=opacity < 0.005)                # every ~100: dead rows move onto live rows, in place
    params = grow(params, count, max_rows=cap)            # every ~100: the same draw, the copies appended

`relocate` and `grow` draw live rows with probability proportional to opacity (`sample_rows`, exact: the same weights
and random words give the same rows on any device and in numpy), correct the opacity and scale of each drawn row and of
its copies so that the rendered result is preserved (`relocation_values`, float64 inside the kernel) and reset the
optimizer state of the rows involved.  Choosing the dead rows and the schedule stays in torch, like the thresholds of
`plan_densify`.  The library has no random numbers: `random` and `noise` are arguments with torch defaults.  Everything
here runs on a HIP device only and never synchronises with the host."""
from __future__ import annotations

import dataclasses
from typing import Optional, Tuple

import torch

from . import _native as nv
from .densify import DensifyPlan, _check_noise, _kernel_moves, densify
from .optim.parameter_class import ParameterClass

_STATE_MODES = ("zero", "sources")
_VALUE_COLUMNS = ("alpha_logit", "log_scaling")
_SHAPE_COLUMNS = ("position", "log_scaling", "rotation", "alpha_logit")
_RANDOM_DTYPES = tuple(d for d in (torch.int64, torch.int32, getattr(torch, "uint32", None)) if d is not None)


@dataclasses.dataclass(frozen=True)
class Relocation:
    """What `relocate` did, on the device: `src_of` (N,) int32, the row every row now is a copy of (itself unless it
    was dead and a live row could be drawn); `copies` (N,) int32, how often each row was drawn."""
    src_of: torch.Tensor
    copies: torch.Tensor


def _check_float(name: str, t, shape, what: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: {name} must be float32, got {t.dtype}")
    if not any(tuple(t.shape) == tuple(s) for s in shape):
        raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected {' or '.join(str(tuple(s)) for s in shape)}")


def _check_mask(name: str, mask, rows: int, what: str) -> None:
    if mask is None:
        return
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(mask).__name__}")
    if mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"{what}: {name} must be a bool or uint8 mask, got {mask.dtype}")
    if tuple(mask.shape) != (rows,):
        raise ValueError(f"{what}: {name} has shape {tuple(mask.shape)}, expected ({rows},)")


def _bytes(mask: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """a bool or uint8 mask as the contiguous bytes the kernels read (a bool tensor stores 0 / 1 bytes)"""
    if mask is None:
        return None
    mask = mask.contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _check_random(random, count: int, what: str) -> None:
    if random is None:
        return
    if not isinstance(random, torch.Tensor):
        raise TypeError(f"{what}: random must be a torch.Tensor, got {type(random).__name__}")
    if random.dtype not in _RANDOM_DTYPES:
        raise TypeError(f"{what}: random must be int64 (values 0 .. 2^32 - 1), int32 or uint32 (all 32 bits), got "
                        f"{random.dtype}")
    if tuple(random.shape) != (count,):
        raise ValueError(f"{what}: random has shape {tuple(random.shape)}, expected ({count},)")


def _random_words(random: Optional[torch.Tensor], count: int, device) -> torch.Tensor:
    """(count,) 32-bit words.  The default is torch.randint(0, 2^32) in int64, the one torch generator call that gives
    all 32 bits, narrowed on the device to the low word of each value; a given int64 tensor is narrowed the same way
    (its values count modulo 2^32), an int32 / uint32 tensor is taken as its bits."""
    if random is None:
        random = torch.randint(0, 2 ** 32, (count,), dtype=torch.int64, device=device)
    if random.dtype == torch.int64:
        return random.contiguous().view(torch.int32)[0::2].contiguous()  # little endian: the low words
    return random.contiguous()


def _draw(weights: torch.Tensor, count: int, random: torch.Tensor, exclude, select) -> Tuple[torch.Tensor, torch.Tensor]:
    n, device = int(weights.shape[0]), weights.device
    rows = torch.empty((count,), dtype=torch.int32, device=device)
    copies = torch.empty((n,), dtype=torch.int32, device=device)
    lib = nv.lib()
    need = lib.gs_sample_rows_scratch_bytes(n)
    scratch = nv.scratch(need, device)
    nv.check(lib.gs_sample_rows(n, nv.ptr(weights), nv.ptr(exclude), count, nv.ptr(random), nv.ptr(select),
                                nv.ptr(rows), nv.ptr(copies), nv.ptr(scratch), need, nv.stream()), "gs_sample_rows")
    return rows, copies


def sample_rows(weights: torch.Tensor, count: Optional[int] = None, *, random: Optional[torch.Tensor] = None,
                exclude: Optional[torch.Tensor] = None,
                select: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`count` (default N) draws with replacement from the N rows, row i with probability proportional to
    floor(clamp(weights[i], 0, 1) * 2^24) -> (rows (count,) int32, copies (N,) int32: how often each row was drawn).

    Exact (gs_sample_rows): integer weights, a uint64 prefix sum, draw j = the first row whose prefix exceeds
    floor(random[j] * total / 2^32); the same arguments give the same rows everywhere.  NaN and negative weights and
    the rows of `exclude` (bool (N,)) are never drawn.  `select` (bool (count,), count == N): only the draws where it
    is set happen, elsewhere rows[j] = j.  Without a drawable row, rows[j] = j and copies = 0.
    random: (count,) int64 with values in 0 .. 2^32 - 1, or int32 / uint32 bit patterns; default
    torch.randint(0, 2**32, dtype=int64) on the device, narrowed there to 32 bits."""
    what = "sample_rows"
    if not isinstance(weights, torch.Tensor):
        raise TypeError(f"{what}: weights must be a torch.Tensor, got {type(weights).__name__}")
    if weights.dtype != torch.float32:
        raise TypeError(f"{what}: weights must be float32, got {weights.dtype}")
    if weights.dim() != 1:
        raise ValueError(f"{what}: weights has shape {tuple(weights.shape)}, expected (N,)")
    n = int(weights.shape[0])
    count = n if count is None else int(count)
    if count < 0 or count >= 2 ** 31 or n >= 2 ** 31:
        raise ValueError(f"{what}: {count} draws from {n} rows (both must stay below 2^31)")
    _check_mask("exclude", exclude, n, what)
    _check_mask("select", select, count, what)
    if select is not None and count != n:
        raise ValueError(f"{what}: a select mask needs count == N ({count} draws, {n} rows)")
    _check_random(random, count, what)
    nv.require_device(weights, what=what)
    nv.require_device(weights, exclude, select, random, dtype=None, what=what)
    if n == 0 and count > 0:
        raise ValueError(f"{what}: {count} draws from an empty table")
    with torch.cuda.device(weights.device):
        return _draw(weights.detach().contiguous(), count, _random_words(random, count, weights.device),
                     _bytes(exclude), _bytes(select))


def _values(opacity: torch.Tensor, log_scaling: torch.Tensor, copies: torch.Tensor,
            min_opacity: float) -> Tuple[torch.Tensor, torch.Tensor]:
    n = int(copies.shape[0])
    alpha_logit, new_scaling = torch.empty_like(opacity), torch.empty_like(log_scaling)
    nv.check(nv.lib().gs_mcmc_relocation_values(n, nv.ptr(opacity), nv.ptr(log_scaling), nv.ptr(copies),
                                                float(min_opacity), nv.ptr(alpha_logit), nv.ptr(new_scaling),
                                                nv.stream()), "gs_mcmc_relocation_values")
    return alpha_logit, new_scaling


def _check_min_opacity(min_opacity, what: str) -> float:
    if not 0.0 < float(min_opacity) < 1.0:
        raise ValueError(f"{what}: min_opacity {min_opacity} not inside (0, 1)")
    return float(min_opacity)


def relocation_values(opacity: torch.Tensor, log_scaling: torch.Tensor, copies: torch.Tensor,
                      min_opacity: float = 0.005) -> Tuple[torch.Tensor, torch.Tensor]:
    """The correction alone: opacity (N,) or (N, 1) float32, log_scaling (N, 3) float32, copies (N,) int32 ->
    (alpha_logit like opacity, log_scaling (N, 3)) of a row and its copies[i] copies, n = min(copies + 1, 51):
        o_new = clamp(1 - (1 - o)^(1 / n), min_opacity, 1 - 2^-23),   alpha_logit = logit(o_new)
        log_scaling += log(o / sum_{i<=n} sum_{k<i} C(i - 1, k) (-1)^k o_new^(k + 1) / sqrt(k + 1))
    evaluated in float64 and rounded once (gs_mcmc_relocation_values).  Rows with copies == 0 are unspecified."""
    what = "relocation_values"
    if not isinstance(copies, torch.Tensor) or copies.dtype != torch.int32 or copies.dim() != 1:
        got = f"{tuple(copies.shape)} {copies.dtype}" if isinstance(copies, torch.Tensor) else type(copies).__name__
        raise TypeError(f"{what}: copies must be an int32 tensor of shape (N,), got {got}")
    n = int(copies.shape[0])
    _check_float("opacity", opacity, ((n,), (n, 1)), what)
    _check_float("log_scaling", log_scaling, ((n, 3),), what)
    min_opacity = _check_min_opacity(min_opacity, what)
    nv.require_device(opacity, log_scaling, what=what)
    nv.require_device(opacity, copies, dtype=None, what=what)
    with torch.cuda.device(opacity.device):
        return _values(opacity.detach().contiguous(), log_scaling.detach().contiguous(), copies.contiguous(),
                       min_opacity)


def _apply(src_of, copies, alpha_logit, new_scaling, out_alpha_logit, out_log_scaling) -> None:
    nv.check(nv.lib().gs_mcmc_apply(int(src_of.shape[0]), nv.ptr(src_of), nv.ptr(copies), nv.ptr(alpha_logit),
                                    nv.ptr(new_scaling), nv.ptr(out_alpha_logit), nv.ptr(out_log_scaling),
                                    nv.stream()), "gs_mcmc_apply")


def _value_columns(params: ParameterClass, what: str) -> Tuple[int, torch.Tensor, torch.Tensor]:
    if not isinstance(params, ParameterClass):
        raise TypeError(f"{what}: params must be a ParameterClass, got {type(params).__name__}")
    missing = [name for name in _VALUE_COLUMNS if name not in params.tensors]
    if missing:
        raise ValueError(f"{what}: needs the columns {list(_VALUE_COLUMNS)}; the table has no {missing}")
    n = int(params.batch_size[0])
    alpha_logit, log_scaling = (params.tensors[name].detach() for name in _VALUE_COLUMNS)
    _check_float("alpha_logit", alpha_logit, ((n,), (n, 1)), what)
    _check_float("log_scaling", log_scaling, ((n, 3),), what)
    return n, alpha_logit, log_scaling


def _relocate_tables(columns, src_of, select, copies) -> None:
    """[(tensor, mode)] changed in place by gs_table_relocate_rows, GS_MOVE_COLUMNS_MAX per launch; a column the kernel
    does not take (not contiguous, rows not a multiple of 4 bytes) goes through torch"""
    n = int(src_of.shape[0])
    batch = []

    def flush():
        if batch:
            arr = (nv.GsRelocateColumn * len(batch))(*batch)
            nv.check(nv.lib().gs_table_relocate_rows(n, nv.ptr(src_of), nv.ptr(select), nv.ptr(copies), len(batch),
                                                     arr, nv.stream()), "gs_table_relocate_rows")
            batch.clear()

    for t, mode in columns:
        t = t.detach()
        if _kernel_moves(t):
            batch.append(nv.GsRelocateColumn(t.data_ptr(), t[0].numel() * t.element_size(), mode))
            if len(batch) == nv.GS_MOVE_COLUMNS_MAX:
                flush()
        elif mode == nv.GS_RELOCATE_COPY:
            t.copy_(t[src_of.long()])  # src_of[j] = j for every row that is not selected
        else:
            rows = copies > 0
            if mode == nv.GS_RELOCATE_ZERO:
                rows = rows | ((select != 0) & (src_of != torch.arange(n, dtype=torch.int32, device=src_of.device)))
            t.masked_fill_(rows.view(n, *([1] * (t.dim() - 1))), 0)
    flush()


def relocate(params: ParameterClass, dead: torch.Tensor, *, random: Optional[torch.Tensor] = None,
             min_opacity: float = 0.005, state: str = "zero") -> Relocation:
    """Move the `dead` rows (bool (N,)) onto live rows, in place: N, the tensors of `params` and those of its
    optimizer state stay what and where they are; there is no host synchronisation.

    Every dead row draws a live row with probability proportional to opacity = torch.sigmoid(alpha_logit)
    (`sample_rows` with exclude = select = dead; random: (N,), only the dead rows' entries are used) and becomes a copy
    of it in every parameter column.  A row drawn c times and its c copies then get the corrected alpha_logit and
    log_scaling of `relocation_values`.  The per-row optimizer state of the dead rows that moved and of the drawn
    rows is zeroed with state="zero"; state="sources" zeroes that of the drawn rows only, as the published MCMC code
    bases do.
    With no live row (all dead, or every live opacity below 2^-24) nothing changes.
    Needs the columns alpha_logit (N, 1) and log_scaling (N, 3), float32."""
    what = "relocate"
    if state not in _STATE_MODES:
        raise ValueError(f"{what}: state must be one of {_STATE_MODES}, got {state!r}")
    n, alpha_logit, log_scaling = _value_columns(params, what)
    if not isinstance(dead, torch.Tensor) or dead.dtype != torch.bool:
        got = dead.dtype if isinstance(dead, torch.Tensor) else type(dead).__name__
        raise TypeError(f"{what}: dead must be a bool tensor, got {got}")
    _check_mask("dead", dead, n, what)
    _check_random(random, n, what)
    min_opacity = _check_min_opacity(min_opacity, what)
    nv.require_device(alpha_logit, log_scaling, what=what)
    nv.require_device(alpha_logit, dead, random, dtype=None, what=what)
    if not (alpha_logit.is_contiguous() and log_scaling.is_contiguous()):
        raise ValueError(f"{what}: alpha_logit and log_scaling must be contiguous (they are corrected in place)")
    device = alpha_logit.device
    if n == 0:
        empty = torch.empty((0,), dtype=torch.int32, device=device)
        return Relocation(empty, empty.clone())
    state_mode = nv.GS_RELOCATE_ZERO if state == "zero" else nv.GS_RELOCATE_ZERO_SOURCES
    columns = [(t, nv.GS_RELOCATE_COPY) for t in params.tensors.values()]
    columns += [(t, state_mode) for table in params.tensor_state.values() for t in table.values()]
    nv.require_device(*(t for t, _ in columns), dtype=None, what=what)
    with torch.cuda.device(device), torch.no_grad():
        opacity = torch.sigmoid(alpha_logit).reshape(n)
        select = _bytes(dead)
        src_of, copies = _draw(opacity, n, _random_words(random, n, device), select, select)
        new_alpha_logit, new_scaling = _values(opacity, log_scaling, copies, min_opacity)
        _relocate_tables(columns, src_of, select, copies)
        _apply(src_of, copies, new_alpha_logit, new_scaling, alpha_logit, log_scaling)
    return Relocation(src_of, copies)


def grow(params: ParameterClass, count: int, *, random: Optional[torch.Tensor] = None, min_opacity: float = 0.005,
         max_rows: Optional[int] = None) -> ParameterClass:
    """`count` new rows (clipped to max_rows - N), each a copy of a row drawn with probability proportional to
    opacity, appended behind the N rows: a new ParameterClass through `densify` (parameter columns copied, optimizer
    state kept for the N rows and zero for the new ones), then the corrected alpha_logit / log_scaling of
    `relocation_values` in every drawn row and its copies.  random: (count,) after clipping.  count <= 0 after
    clipping, or an empty table, returns `params` itself.  No host synchronisation."""
    what = "grow"
    n, alpha_logit, log_scaling = _value_columns(params, what)
    count = int(count)
    if max_rows is not None:
        count = min(count, int(max_rows) - n)
    min_opacity = _check_min_opacity(min_opacity, what)
    if count <= 0 or n == 0:
        return params
    if n + count >= 2 ** 31:
        raise ValueError(f"{what}: {n} + {count} rows (must stay below 2^31)")
    _check_random(random, count, what)
    nv.require_device(alpha_logit, log_scaling, what=what)
    nv.require_device(alpha_logit, random, dtype=None, what=what)
    device = alpha_logit.device
    with torch.cuda.device(device), torch.no_grad():
        opacity = torch.sigmoid(alpha_logit).reshape(n).contiguous()
        drawn, copies = _draw(opacity, count, _random_words(random, count, device), None, None)
        src_of = torch.cat([torch.arange(n, dtype=torch.int32, device=device), drawn])
        grown = densify(params, DensifyPlan(src_of, n, count, 0, n + count, 2, n), state="zero")
        new_alpha_logit, new_scaling = _values(opacity, log_scaling.contiguous(), copies, min_opacity)
        _apply(src_of, copies, new_alpha_logit, new_scaling, grown.tensors["alpha_logit"].detach(),
               grown.tensors["log_scaling"].detach())
    return grown


def perturb(gaussians, lr: float, *, noise: Optional[torch.Tensor] = None, noise_lr: float = 5e5, k: float = 100.0,
            x0: float = 0.995) -> None:
    """position += R S^2 R^T (noise * g * lr * noise_lr), g = sigmoid(k ((1 - opacity) - x0)), in place on the
    `position` column of a ParameterClass, a Gaussians3D or any mapping with position (N, 3), log_scaling (N, 3),
    rotation (N, 4, xyzw) and alpha_logit (N, 1), all float32 (gs_mcmc_perturb: one launch, no autograd).
    noise: (N, 3) float32, default torch.randn on the device.  Rows whose gate is exactly zero (opacity above 0.89
    with the defaults) and rows with zero noise keep their position bits; the former cost 4 bytes of traffic each.
    Call it between the optimizer step and the next forward."""
    what = "perturb"
    if not hasattr(gaussians, "items"):
        raise TypeError(f"{what}: expected a ParameterClass, a Gaussians3D or a mapping of columns, got "
                        f"{type(gaussians).__name__}")
    table = dict(gaussians.items())
    missing = [name for name in _SHAPE_COLUMNS if name not in table]
    if missing:
        raise ValueError(f"{what}: needs the columns {list(_SHAPE_COLUMNS)}; the table has no {missing}")
    position, log_scaling, rotation, alpha_logit = (table[name].detach() if isinstance(table[name], torch.Tensor)
                                                    else table[name] for name in _SHAPE_COLUMNS)
    n = int(position.shape[0]) if isinstance(position, torch.Tensor) and position.dim() > 0 else 0
    _check_float("position", position, ((n, 3),), what)
    _check_float("log_scaling", log_scaling, ((n, 3),), what)
    _check_float("rotation", rotation, ((n, 4),), what)
    _check_float("alpha_logit", alpha_logit, ((n, 1), (n,)), what)
    _check_noise(noise, (n, 3), what)
    nv.require_device(position, log_scaling, rotation, alpha_logit, noise, what=what)
    if not position.is_contiguous():
        raise ValueError(f"{what}: position must be contiguous (it is changed in place)")
    if n == 0:
        return
    device = position.device
    with torch.cuda.device(device), torch.no_grad():
        if noise is None:
            noise = torch.randn((n, 3), dtype=torch.float32, device=device)
        nv.check(nv.lib().gs_mcmc_perturb(n, nv.ptr(position), nv.ptr(log_scaling.contiguous()),
                                          nv.ptr(rotation.contiguous()), nv.ptr(alpha_logit.contiguous()),
                                          nv.ptr(noise.detach().contiguous()), float(lr) * float(noise_lr), float(k),
                                          float(x0), nv.stream()), "gs_mcmc_perturb")


__all__ = ["Relocation", "grow", "perturb", "relocate", "relocation_values", "sample_rows"]
