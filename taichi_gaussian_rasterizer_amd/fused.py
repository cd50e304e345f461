"""Fused frame: the whole render_gaussians pipeline as ONE autograd node.

Same kernels as the operator-by-operator composition in renderer.py, but enqueued back to back
on the stream with the intermediate counts (visible Gaussians V, overlaps K) left on the device:

  * no host read-back between the stages -- the single synchronisation is at the END of the forward,
    when the tensor shapes of the result (V rows) have to be known to Python;
  * no torch glue on the path: the SH colours and the depth features are written straight into the
    rasterizer's feature rows, the rasterizer's 64-byte gradient rows are consumed in place by the SH
    and projection backward (no unpack, no cat/index backward, no zero-filled dense temporaries);
  * the whole forward is one gs_frame_fwd call into one workspace, the backward one gs_frame_bwd call (a sharded
    frame's backward is three: its gradient exchange sits between the rasterizer and the adjoints);
  * the pair / overlap buffers are sized from the largest K seen for the shape (x1.25, in classes of 65 536; the first
    frame of a shape gets the smallest class); the mapper clamps to the capacity and raises a flag, in which case the
    frame is re-run once with room for the K it counted.

This is SURVEY.md 8(f)-1: in the reference that glue is ~24 % of the forward+backward GPU time
(profiles/bicycle_2048.txt:38,42,44,47).  Results are bit-identical to the composed operators.
"""
from __future__ import annotations

import ctypes
import weakref

import torch

from . import _native as nv
from .data_types import RasterConfig
from .spherical_harmonics import check_sh_degree

_K_HINT = {}  # (n, w, h, tile_size, use_depth16) -> (max overlaps, max tile population) seen for that shape
# the backward of an unsharded frame: true = one gs_frame_bwd call, False = the three calls a sharded frame makes
# around its exchange (tests/conftest.py frame_path runs the fused-frame tests both ways)
FRAME_CALLS = True
_PINNED = {}  # device index -> ring of pinned int32[8] host buffers for the asynchronous count read-back


def _pinned_counts(dev: torch.device) -> torch.Tensor:
    ring = _PINNED.get(dev.index)
    if ring is None:
        ring = _PINNED[dev.index] = dict(bufs=[torch.empty((8,), dtype=torch.int32).pin_memory() for _ in range(4)],
                                         at=0)
    ring["at"] = (ring["at"] + 1) % len(ring["bufs"])
    return ring["bufs"][ring["at"]]


_EVENTS = {}   # device index -> ring of (torch.cuda.Event, raw handle)
_EMPTY = {}    # (device, shape) -> cached empty placeholder outputs
_FRAMES = {}   # frame key -> (GsFrame, GsFrameLayout)
# sparse_grad: data_ptr of the index list of a frame's sparse gradients -> (weak reference to its storage, its length).
# The optimizers trust a list found here to be ascending and distinct (it is a copy of points_in_view).  AccumulateGrad
# keeps the storage of a gradient it stores first, so .grad._indices() is recognised by address; whatever autograd
# builds from several gradients has storage of its own and is not.
_SPARSE_INDEXES = {}


class _Overflow(Exception):
    pass


def _register_sparse_indexes(idx: torch.Tensor) -> None:
    for ptr in [ptr for ptr, (ref, _) in _SPARSE_INDEXES.items() if ref() is None]:
        del _SPARSE_INDEXES[ptr]
    if idx.numel() > 0:
        _SPARSE_INDEXES[idx.data_ptr()] = (weakref.ref(idx.untyped_storage()), idx.numel())


def is_frame_sparse_grad(grad: torch.Tensor) -> bool:
    """whether a sparse gradient is the one a single backward of a sparse_grad frame produced -- its indices are then
    ascending and distinct although autograd has dropped the is_coalesced flag.  No device work."""
    idx = grad._indices()
    hit = _SPARSE_INDEXES.get(idx.data_ptr()) if idx.numel() > 0 else None
    if hit is None or idx.dim() != 2 or idx.shape[0] != 1 or hit[1] != idx.shape[1]:
        return False
    storage = hit[0]()  # alive: the address has not been handed to another tensor since
    return storage is not None and storage._cdata == idx.untyped_storage()._cdata


def _remember(key, K, max_tile):
    hint = _K_HINT.get(key)
    _K_HINT[key] = (max(K, hint[0]) if hint else K, max(max_tile, hint[1]) if hint else max_tile)


def _carve(base, offset, shape):
    """row-major view of `shape` at byte `offset` of the frame call's workspace, `base` = the workspace viewed as the
    element type"""
    strides, acc = [], 1
    for s in reversed(shape):
        strides.append(acc)
        acc *= s
    return base.as_strided(shape, tuple(reversed(strides)), offset // base.element_size()).detach()


def _empty(dev, shape):
    key = (dev, shape)
    t = _EMPTY.get(key)
    if t is None:
        t = _EMPTY[key] = torch.empty(shape, dtype=torch.float32, device=dev)
    return t


def _exchange_ranks(shard, exchange, group, n, owned_range):
    """(world, rank) of a sharded frame's sparse exchange, (0, 0) when there is none"""
    if shard is None or exchange != "sparse":
        return 0, 0
    import torch.distributed as dist

    from . import parallel
    if dist.is_initialized():
        return dist.get_world_size(group), dist.get_rank(group)
    world = max(parallel.EMULATED_WORLD, 1)
    rank = 0 if owned_range is None else owned_range[0] // max(-(-n // world), 1)
    return world, rank


def _start_sparse_exchange(meta, world, touched, counts, owned_rows):
    """Bookkeeping of a sharded frame's sparse exchange, done during the FORWARD: keep the list of the splats that can
    reach this rank's rows, which gs_frame_fwd left in the workspace (ascending rows, so that the entries of one owner
    are contiguous; it also evaluated the colours of exactly these rows), and start the all-gather of the list lengths
    (grad_mode "sharded": of the per-owner counts).  The backward finds both in `meta`."""
    from . import parallel
    M = meta["touched_count"]
    sharded = meta["grad_mode"] == "sharded"
    if not sharded:
        counts = torch.full((1,), M, dtype=torch.int64, device=touched.device)
    # a rank without tile rows or without a list has no range of rows to merge into: it merges every row
    meta["owned_rows"] = owned_rows if (sharded and meta["num_tiles"] > 0 and M > 0) else None
    meta["touched"] = touched
    meta["sizes"] = parallel.SizesFuture(counts, meta["group"]) if world > 1 else None


# ---------------------------------------------------------------------------------------------------------------
# One C-ABI call per direction (include/gsplat_hip.h gs_frame_fwd / gs_frame_bwd): every stage of the frame, enqueued
# from a single host call into one workspace whose sub-buffers are carved by offset.  Every frame's forward is such a
# call, sized by the overlap count seen for its shape (none yet: the smallest class); a frame with more overlaps than
# its capacity is run once more with room for them (render_fused).

def _frame_for(n, C, degree, w, full_h, depth_range, render_depth, use_depth16, render_median, prepare_backward,
               k_cap, tile_hint, shard, config, exchange_world=0, exchange_rank=0):
    key = (n, C, degree, w, full_h, float(depth_range[0]), float(depth_range[1]), render_depth, use_depth16,
           render_median, prepare_backward, k_cap, tile_hint, shard, config, nv.TUNING["wave_sub_blocks"],
           nv.TUNING["no_heavy_split"], exchange_world, exchange_rank)
    hit = _FRAMES.get(key)
    if hit is None:
        frame = nv.GsFrame()
        frame.n, frame.channels, frame.sh_degree, frame.width, frame.height = n, C, degree, w, full_h
        frame.near_plane, frame.far_plane = float(depth_range[0]), float(depth_range[1])
        frame.render_depth, frame.use_depth16 = int(render_depth), int(use_depth16)
        frame.render_median_depth, frame.prepare_backward = int(render_median), int(prepare_backward)
        frame.k_capacity, frame.max_tile_hint = int(k_cap), int(tile_hint)
        frame.has_shard = 0 if shard is None else 1
        if shard is not None:
            frame.shard = nv.GsRowShard(int(shard.row_begin), int(shard.row_end), int(shard.band), int(shard.period),
                                        int(shard.phase))
        frame.cfg = nv.make_config(config)
        frame.depth_forward_cut = nv.make_config(config, cut_scale=float(depth_range[1]) ** 2).forward_cut
        frame.exchange_world, frame.exchange_rank = int(exchange_world), int(exchange_rank)
        layout = nv.GsFrameLayout()
        nv.check(nv.lib().gs_frame_layout(ctypes.byref(frame), ctypes.byref(layout)), "gs_frame_layout")
        if len(_FRAMES) > 256:
            _FRAMES.clear()
        hit = _FRAMES[key] = (frame, layout)
    return hit


def _counts_event(dev: torch.device):
    ring = _EVENTS.get(dev.index)
    if ring is None:
        evs = []
        for _ in range(4):
            ev = torch.cuda.Event()
            ev.record()  # creates the underlying hipEvent_t, whose handle the library records later
            evs.append((ev, ctypes.c_void_p(ev.cuda_event)))
        ring = _EVENTS[dev.index] = dict(evs=evs, at=0)
    ring["at"] = (ring["at"] + 1) % len(ring["evs"])
    return ring["evs"][ring["at"]]


def _forward_call(m, inputs, needs_grad, depth_range, use_depth16, render_median, key, k_cap, tile_hint, world,
                  rank, background=None):
    """fills the frame by one gs_frame_fwd call into a workspace sized for k_cap overlaps (raises _Overflow when the
    frame has more); returns its outputs, the workspace and, for a sparse exchange, the lists gs_frame_fwd prepared"""
    position, log_scaling, rotation, alpha_logit, feature, T, proj = inputs
    lib = nv.lib()
    dev = position.device
    n, w, full_h, C, config, shard = m["n"], m["w"], m["full_h"], m["C"], m["config"], m["shard"]
    render_depth = m["render_depth"]
    # a sharded frame's backward is split at its exchange, and the split calls clear their own rows
    prepare_backward = needs_grad and shard is None and bool(FRAME_CALLS)
    frame, L = _frame_for(n, C, m["degree"], w, full_h, depth_range, render_depth, use_depth16, render_median,
                          prepare_backward, k_cap, tile_hint, shard, config, world, rank)
    ws = torch.empty((L.workspace_bytes,), dtype=torch.uint8, device=dev)
    scratch = torch.empty((L.fwd_scratch_bytes,), dtype=torch.uint8, device=dev)
    host_counts = _pinned_counts(dev)
    ready, ready_handle = _counts_event(dev)
    nv.check(lib.gs_frame_fwd(ctypes.byref(frame), nv.ptr(position), nv.ptr(log_scaling), nv.ptr(rotation),
                              nv.ptr(alpha_logit), nv.ptr(feature), nv.ptr(T), nv.ptr(proj), nv.ptr(ws),
                              L.workspace_bytes, nv.ptr(scratch), L.fwd_scratch_bytes, nv.ptr(host_counts),
                              ready_handle, nv.stage_events(nv.FRAME_FWD_STAGES), nv.ptr(background), nv.stream()),
             "gs_frame_fwd")
    ready.synchronize()  # waits for the mapper's scan only, not for the rasterizer
    host = host_counts.tolist()
    K, max_tile, overflow, V = host[0], host[1], host[2], host[4]
    _remember(key, K, max_tile)
    if overflow:  # more overlaps than the capacity: the caller runs the frame again, sized for the K just recorded
        raise _Overflow()

    F, h = L.num_features, L.local_height
    num_tiles = max(L.tiles_x * L.tiles_y, 0)
    M = int(host[5]) if num_tiles > 0 else 0
    # rows_clean: gs_frame_fwd has zero-filled the gradient rows gs_frame_bwd accumulates into
    m.update(V=V, K=K, F=F, col0=F - C, num_tiles=num_tiles, touched_count=M, frame=(frame, L),
             rows_clean=prepare_backward)
    f32, i32, i64 = ws.view(torch.float32), ws.view(torch.int32), ws.view(torch.int64)
    image = _carve(f32, L.image, (h, w, F))
    outs = (_carve(f32, L.out_image, (h, w, C)) if render_depth else image, _carve(f32, L.alpha, (h, w)),
            _carve(f32, L.points, (V, 7)), _carve(f32, L.depth, (V, 1)), _carve(i64, L.indexes, (V,)),
            _carve(f32, L.visibility, (V,)) if config.compute_visibility else None,
            _carve(f32, L.img_depth, (h, w)) if render_depth else None,
            _carve(f32, L.img_var, (h, w)) if render_depth else None,
            _carve(f32, L.median, (h, w)) if render_median else None)
    lists = None
    if shard is not None and m["exchange"] == "sparse":
        # the frame call has already compacted the list (ascending rows) and cut it by owner; owned_rows = counts[2:4]
        lists = (_carve(i32, L.touched, (M,)), _carve(i64, L.owner_counts, (world,)), _carve(i32, L.counts + 8, (2,)))
    return outs, ws, lists


def _forward(ctx, needs, position, log_scaling, rotation, alpha_logit, feature, T_camera_world, projection, image_size,
             depth_range, config: RasterConfig, render_depth: bool, use_depth16: bool, render_median: bool, shard,
             group, holder, exchange: str, grad_mode: str, owned_range, sparse_grad: bool, key, k_cap: int,
             tile_hint: int, background=None, differentiable_weight: bool = False):
    """the forward of the frame node; `needs`: which of the seven tensors get a gradient"""
    nv.require_device(position, log_scaling, rotation, alpha_logit, feature, T_camera_world, projection, background,
                      what="render_gaussians")
    background = None if background is None else background.contiguous()
    inputs = (position, log_scaling, rotation, alpha_logit, feature, T_camera_world.contiguous(),
              projection.contiguous())
    dev = position.device
    n = position.shape[0]
    world, rank = _exchange_ranks(shard, exchange, group, n, owned_range)
    m = dict(n=n, w=int(image_size[0]), full_h=int(image_size[1]), C=feature.shape[1],
             degree=check_sh_degree(feature) if feature.dim() == 3 else -1,  # -1: plain (N, C) features, no SH
             config=config, render_depth=render_depth, group=group, shard=shard, exchange=exchange,
             grad_mode=grad_mode, owned_range=owned_range, rank=rank, sparse_grad=sparse_grad,
             weight_grad=bool(differentiable_weight))
    outs, ws, lists = _forward_call(m, inputs, any(needs), depth_range, use_depth16, render_median, key, k_cap,
                                    tile_hint, world, rank, background)
    out_image, alpha, points_v, depth_v, indexes_v, vis_out, img_depth, img_var, median = outs

    vis_out, img_depth, img_var, median = (_empty(dev, (0,)) if t is None else t
                                           for t in (vis_out, img_depth, img_var, median))
    heur = torch.zeros((m["V"], 2), dtype=torch.float32, device=dev) if config.compute_point_heuristic \
        else _empty(dev, (0, 2))
    if lists is not None:
        _start_sparse_exchange(m, world, *lists)
    if holder is not None and shard is not None:
        holder["touched_count"] = m["touched_count"]
    ctx.meta = m
    ctx.camera_grads = (needs[5], needs[6])
    ctx.heur = heur
    ctx.holder = holder
    # outputs nobody differentiates through (projected splats, depths) must not cost zero-filled gradients
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(*inputs, ws)
    ctx.mark_non_differentiable(indexes_v, vis_out, heur, median)
    if not differentiable_weight:
        ctx.mark_non_differentiable(alpha)
    if not render_depth:
        ctx.mark_non_differentiable(img_depth, img_var)
    return out_image, alpha, points_v, depth_v, indexes_v, vis_out, heur, img_depth, img_var, median


def _publish(ctx, rows, V, attached=None):
    """`Rendering.gaussians2d` is an OUTPUT of the frame node, so autograd alone would leave its .grad without the
    rasterizer's dL/d(splat) (which never leaves the node).  The reference feeds that very tensor to rasterize, so
    `gaussians2d.retain_grad()` + `viewspace_gradient` (renderer.py:234-239) is the classic densification signal there:
    add the rasterizer's part (summed over the ranks of a sharded frame) to what the retain_grad hook has stored (this
    pass's upstream gradient, earlier backward passes) -- .grad accumulates over several backward passes as it does in
    the reference, and an empty view gets (0, 7).  `attached`: the gradient the rows hold besides the rasterizer's
    (the retain_grad hook has stored that part already)."""
    out = ctx.holder.get("gaussians2d") if ctx.holder else None
    out = out() if out is not None else None
    if out is not None and out.retains_grad:
        part = rows[:V, :7].clone() if V > 0 else rows.new_zeros((0, 7))
        if attached is not None:
            part -= attached
        out.grad = part if out.grad is None else out.grad + part


def _add_centre_grad(d_T, d_centre, T):
    """Y = T^-1, dL/dT = -Y^T (dL/dY) Y^T with dL/dY zero except the centre column"""
    if d_centre is None:
        return d_T
    with torch.no_grad():
        Y = torch.linalg.inv(T.detach().cpu().double())
        dY = torch.zeros((4, 4), dtype=torch.float64)
        dY[:3, 3] = d_centre.cpu().double()
        return d_T + (-(Y.T @ dY @ Y.T)).to(device=d_T.device, dtype=torch.float32)


def _exchange(m, rows, feats):
    """a sharded frame's partial gradients, summed over the ranks: (colour columns (V', C), splat [+ depth feature]
    columns (V', 7 + col0), the handle of a collective still in flight or None), V' = max(V, 1); `feats`: the frame's
    feature rows, whose SH clamp mask the packs apply (only the ranks that rasterized a splat know it)"""
    from . import parallel
    lib, dev, s = nv.lib(), rows.device, nv.stream()
    F, C, col0 = m["F"], m["C"], m["col0"]
    rows_n = rows.shape[0]
    pf = torch.empty((rows_n, C), dtype=torch.float32, device=dev)
    pp = torch.empty((rows_n, 7 + col0), dtype=torch.float32, device=dev)
    if m.get("sizes") is None:
        # Every rank rendered different rows: the per-Gaussian partial gradients are summed over the ranks, 4*(7+F)
        # bytes per visible Gaussian in all.  Two collectives, colour columns first: the SH adjoint only needs those and
        # runs while the splat columns are still in flight.
        nv.check(lib.gs_shard_pack_grads(rows_n, F, col0, nv.ptr(rows), feats, nv.ptr(pf), nv.ptr(pp), s),
                 "gs_shard_pack_grads")
        return pf, pp, parallel._reduce_partial_gradients(pf, pp, m["group"])
    # Sparse exchange (parallel.py): one entry [row, 7 + F gradient words] per splat that can reach this rank's rows --
    # the mapper's own list -- instead of the dense rows, 7/8 of which are zeros on every rank of 8.
    touched, M = m["touched"], int(m["touched"].shape[0])
    entries = torch.empty((max(M, 1), parallel.ENTRY_HEAD + F), dtype=torch.float32, device=dev)
    nv.check(lib.gs_shard_pack_sparse(M, nv.ptr(touched), F, col0, nv.ptr(rows), feats, nv.ptr(entries), s),
             "gs_shard_pack_sparse")
    table = m["sizes"].result()
    group, rank = m["group"], m["rank"]
    if m["grad_mode"] == "sharded":   # table[q][r] = entries rank q holds for owner r
        lists = parallel.exchange_entries_sharded(entries, [int(x) for x in table[rank]],
                                                  [int(table[q][rank]) for q in range(len(table))], group)
    else:                             # table[q][0] = list length of rank q
        lists = parallel.exchange_entries_replicated(entries, M, [int(t[0]) for t in table], group)
    # every list in one pass over the dense rows (rank order inside each tile: the same sums on every rank; every row is
    # written, so no clearing)
    nl = len(lists)
    ptrs = (ctypes.c_void_p * nl)(*[ent.data_ptr() if cnt else None for ent, cnt in lists])
    cnts = (ctypes.c_int64 * nl)(*[cnt for _, cnt in lists])
    tmp_bytes = 4 * nl * (-(-rows_n // 256) + 1)
    tmp = torch.empty((tmp_bytes,), dtype=torch.uint8, device=dev)
    nv.check(lib.gs_shard_merge_sparse(nl, ptrs, cnts, F, col0, rows_n, nv.ptr(pf), nv.ptr(pp),
                                       nv.ptr(m.get("owned_rows")), nv.ptr(tmp), tmp_bytes, s), "gs_shard_merge_sparse")
    return pf, pp, None


def _backward(ctx, g_image, g_points, g_depth, g_img_depth, g_img_var, g_alpha=None):
    """the seven input gradients of the frame; with sparse_grad the five of the Gaussians as sparse tensors over
    points_in_view (_backward_rows, _as_sparse)"""
    saved = ctx.saved_tensors  # read before the backward: a second pass (retain_graph) clears rows of the workspace
    outs, d_T, d_proj = _backward_rows(ctx, g_image, g_points, g_depth, g_img_depth, g_img_var, g_alpha)
    if ctx.meta["sparse_grad"]:
        m = ctx.meta
        outs = _as_sparse(outs, saved[:5], saved[7], m["frame"][1], m["V"])
    return (*outs, d_T, d_proj)


def _backward_rows(ctx, g_image, g_points, g_depth, g_img_depth, g_img_var, g_alpha=None):
    """the frame's backward on the workspace of its gs_frame_fwd: one gs_frame_bwd call when the forward prepared it,
    otherwise three -- rasterizer, colour adjoint, projection adjoint -- with a sharded frame's exchange of its partial
    gradients after the first; returns (the five Gaussian gradients, dL/dT, dL/dprojection), the five row-compact with
    sparse_grad: (max(V, 1), ...) pieces of one allocation, row i the gradient of Gaussian points_in_view[i].  g_alpha:
    the gradient of image_weight of a frame rendered with differentiable_weight (the rasterizer's backward takes it into
    every pixel's initial R; the divisor of depth / depth_var stays a constant).  `ctx`: anything that carries the
    frame's meta, camera_grads, heur, holder and saved_tensors (_FrameRender's context, a _View of _ViewsRender)"""
    saved = ctx.saved_tensors
    inputs, ws = saved[:7], saved[7]
    position, log_scaling, rotation, alpha_logit, feature, T, proj = inputs
    m = ctx.meta
    frame, L = m["frame"]
    lib = nv.lib()
    dev = position.device
    n, V, K, F = m["n"], m["V"], m["K"], m["F"]
    RS = L.grad_row_floats
    scratch = torch.empty((L.bwd_scratch_bytes,), dtype=torch.uint8, device=dev)
    whole = bool(frame.prepare_backward)  # the forward has zero-filled gradient rows in the workspace
    base, off = (ws, L.grad_rows) if whole else (scratch, L.b_grad_rows)
    rows = base.view(torch.float32).as_strided((max(V, 1), RS), (RS, 1), off // 4)
    if whole and not m["rows_clean"]:
        rows.zero_()  # a second backward through the same frame (retain_graph): the rows hold the first one's sums
    m["rows_clean"] = False
    gi = gd_ = gv_ = None
    if g_image is not None:
        gi = g_image.contiguous()
    if m["render_depth"]:
        gd_ = g_img_depth.contiguous() if g_img_depth is not None else None
        gv_ = g_img_var.contiguous() if g_img_var is not None else None
    att_p = g_points.contiguous() if (g_points is not None and V > 0) else None
    att_d = g_depth.contiguous() if (g_depth is not None and V > 0) else None
    gw = g_alpha.contiguous() if (g_alpha is not None and m["weight_grad"]) else None
    if gw is not None and gi is None and gd_ is None and gv_ is None:
        gi = torch.zeros((L.local_height, m["w"], m["C"]), dtype=torch.float32, device=dev)  # only the weight has a gradient
    nv.require_device(gi, gd_, gv_, att_p, att_d, gw, what="render_gaussians backward")
    need_T, need_proj = ctx.camera_grads
    # grad_mode "sharded": the adjoints run on this rank's index range [lo, hi) only and the gradients come out
    # range-shaped; one allocation for the five parameter gradients
    lo, hi = m["owned_range"] if m["owned_range"] is not None else (0, n)
    nr = hi - lo
    # sparse_grad: the adjoints write one row per VISIBLE Gaussian (gs_frame_bwd_rows); nothing of size n is allocated
    compact = m["sparse_grad"]
    out_rows = max(V, 1) if compact else nr
    params = (position, log_scaling, rotation, alpha_logit, feature)
    sizes = [t.numel() if out_rows == n else t.numel() // n * out_rows for t in params]
    # the compact pieces start on 256-byte boundaries whatever V is: the SH adjoint writes its rows with 16-byte stores,
    # and a wave of the optimizer step reads 256 contiguous bytes of a piece
    starts, at = [], 0
    for sz in sizes:
        starts.append(at)
        at += -(-sz // 64) * 64 if compact else sz
    flat = torch.empty((at,), dtype=torch.float32, device=dev)
    outs = [flat.as_strided(t.shape if out_rows == n else (out_rows, *t.shape[1:]), t.stride(), start)
            for t, start in zip(params, starts)]
    frame_bwd = lib.gs_frame_bwd_rows if compact else lib.gs_frame_bwd
    d_T = torch.empty((4, 4), dtype=torch.float32, device=dev) if need_T else None
    d_proj = torch.empty((4,), dtype=torch.float32, device=dev) if need_proj else None
    d_centre = None
    if m["degree"] >= 1 and need_T:
        d_centre = torch.zeros((3,), dtype=torch.float32, device=dev)

    def call(stages=None, colours=None, splats=None):
        # stages None: the whole backward; colours / splats: the summed partial gradients of a sharded frame
        part = None if stages is None else ctypes.byref(nv.GsFrameBwdPart(
            stages.start, stages.stop, None if colours is None else colours.data_ptr(),
            None if splats is None else splats.data_ptr(), 0 if colours is None else colours.stride(0),
            0 if splats is None else splats.stride(0), lo, hi))
        nv.check(frame_bwd(ctypes.byref(frame), *map(nv.ptr, inputs), nv.ptr(ws), L.workspace_bytes,
                           nv.ptr(scratch), L.bwd_scratch_bytes, V, K, nv.ptr(gi), nv.ptr(gd_), nv.ptr(gv_),
                           nv.ptr(gw), nv.ptr(att_p), nv.ptr(att_d), *map(nv.ptr, outs), nv.ptr(d_T), nv.ptr(d_proj),
                           nv.ptr(d_centre), nv.stage_events(nv.FRAME_BWD_STAGES, stages), part, nv.stream()),
                 "gs_frame_bwd_rows" if compact else "gs_frame_bwd")

    call(None if whole else range(nv.GS_BWD_RASTER, nv.GS_BWD_COLOURS))
    if m["config"].compute_point_heuristic and V > 0:
        ctx.heur.copy_(rows[:V, 7 + F:9 + F])
    if whole:
        _publish(ctx, rows, V, att_p)  # the rows hold the attached gradient as well
    else:
        pf = pp = wait = None
        if m["shard"] is not None:
            feats = ctypes.c_void_p(ws.data_ptr() + L.features) if m["degree"] >= 0 else None
            pf, pp, wait = _exchange(m, rows, feats)
        call(range(nv.GS_BWD_COLOURS, nv.GS_BWD_PROJECT), colours=pf)
        if wait is not None:
            wait.wait()
        _publish(ctx, rows if pp is None else pp, V)  # before the PROJECT call adds the attached gradient
        call(range(nv.GS_BWD_PROJECT, nv.GS_BWD_STAGES), splats=pp)
    return outs, _add_centre_grad(d_T, d_centre, T), d_proj


def _as_sparse(rows, params, ws, L, V):
    """the five row-compact gradients as hybrid COO tensors over one fresh copy of points_in_view (a copy, so that
    .grad does not keep the frame's workspace alive)"""
    idx = _carve(ws.view(torch.int64), L.indexes, (V,)).clone().view(1, V)
    _register_sparse_indexes(idx)
    return [torch.sparse_coo_tensor(idx, r[:V], t.shape, is_coalesced=True) for r, t in zip(rows, params)]


_BACKGROUND_ARG = 23  # position of `background` among the arguments of _forward behind ctx and needs


def _background_grad(ctx, g_image):
    """dL/dbackground_c = sum over the pixels of g_c T with T = 1 - image_weight, in torch on the stream: off the default
    path, and without a host synchronisation"""
    m = ctx.meta
    C = m["C"]
    if g_image is None:
        return torch.zeros((C,), dtype=torch.float32, device=ctx.saved_tensors[0].device)
    L = m["frame"][1]
    alpha = _carve(ctx.saved_tensors[7].view(torch.float32), L.alpha, (L.local_height, m["w"]))
    return (g_image * (1.0 - alpha).unsqueeze(-1)).sum((0, 1))


class _FrameRender(torch.autograd.Function):
    """the whole frame as one autograd node; forward arguments: see _forward"""

    @staticmethod
    @nv.on_tensor_device
    def forward(ctx, *args):
        return _forward(ctx, ctx.needs_input_grad[:7], *args)

    @staticmethod
    @nv.on_tensor_device
    def backward(ctx, g_image, g_alpha, g_points, g_depth, _g_idx, _g_vis, _g_heur, g_img_depth, g_img_var,
                 _g_median=None):
        d = _backward(ctx, g_image, g_points, g_depth, g_img_depth, g_img_var, g_alpha)
        rest = [None] * (len(ctx.needs_input_grad) - len(d))
        if len(rest) > _BACKGROUND_ARG - 7 and ctx.needs_input_grad[_BACKGROUND_ARG]:
            rest[_BACKGROUND_ARG - 7] = _background_grad(ctx, g_image)
        return d + tuple(rest)


class _OwnedRender(torch.autograd.Function):
    """grad_mode "sharded" (parallel.py): the replicated Gaussians are DATA here; what is differentiated are this rank's
    own rows [lo, hi) of them, held as separate leaf tensors by a sharded optimizer (`owned`: their values are taken to
    be the corresponding rows of the replicated tensors).  Forward: the sharded frame as usual.  Backward: partial
    gradients go to their owners through one all-to-all, the SH / projection adjoints run on the owned range only and
    the gradients come out range-shaped -- no all-gather of gradients, no (N, ...) zero rows written."""

    @staticmethod
    @nv.on_tensor_device
    def forward(ctx, o_position, o_log_scaling, o_rotation, o_alpha_logit, o_feature, full, rest):
        return _forward(ctx, (True,) * 5 + (False, False), *full, *rest)

    @staticmethod
    @nv.on_tensor_device
    def backward(ctx, *grads):
        return _FrameRender.backward(ctx, *grads)[:5] + (None,) * (len(ctx.needs_input_grad) - 5)


class _View:
    """What _forward leaves on an autograd context and _backward_rows reads there, for ONE view of _ViewsRender: the
    views' tensors are all saved on that node's own context, which hands a view its eight before the view's backward."""

    def __init__(self):
        self.saved_tensors = ()
        self.non_differentiable = []

    def set_materialize_grads(self, value):
        pass  # the node's own context

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *tensors):
        self.non_differentiable.extend(tensors)


_VIEW_OUTPUTS = 10   # of _forward, per view
_VIEWS_CAMERAS = 7   # position of the first camera matrix among the arguments of _ViewsRender.forward behind ctx


def _view_tables(entries):
    """the host table of gs_views_sum_rows from (workspace, layout, values, count, stride) per view.  The caller keeps
    the tensors referenced until the launch has been issued."""
    table = (nv.GsViewRows * max(len(entries), 1))()
    for k, (ws, L, values, count, stride) in enumerate(entries):
        table[k] = nv.GsViewRows(ws.data_ptr() + L.slot_of, values.data_ptr() if count > 0 else None, count, stride)
    return table


class _ViewsRender(torch.autograd.Function):
    """B frames of the same Gaussians as ONE autograd node (renderer.render_views).  Forward: one gs_frame_fwd per view
    as in _FrameRender, then the union of the views' visible rows from the workspaces' slot_of tables (gs_views_union)
    and, with compute_visibility, the visibility summed over the views (gs_views_sum_rows); one host read for the size
    of the union.  Backward: the frame backward of every view that received a gradient, into its own row-compact
    pieces, then one gs_views_sum_rows per parameter over all those views at once, on the union's rows: the sum in
    view order, no sort, no search, nothing through autograd's sparse `+`.
    Memory: the B workspaces stay alive until the backward, and during it the compact gradient rows of all views
    (sum of V_b rows) and the merged ones (U rows) exist side by side.
    forward(position, log_scaling, rotation, alpha_logit, feature, spec, background, T_0, projection_0, T_1, ...);
    returns the ten outputs of _forward for every view, then the union (U) int64 and its summed visibility."""

    @staticmethod
    @nv.on_tensor_device
    def forward(ctx, position, log_scaling, rotation, alpha_logit, feature, spec, background, *cameras):
        params = (position, log_scaling, rotation, alpha_logit, feature)
        needs = ctx.needs_input_grad
        lib, dev, n = nv.lib(), position.device, position.shape[0]
        views, outs, saved = [], [], []
        for b, (image_size, depth_range, holder, key) in enumerate(spec["frames"]):
            view = _View()
            at = _VIEWS_CAMERAS + 2 * b
            view_needs = (*needs[:5], needs[at], needs[at + 1])
            colour = background if background is None or background.dim() == 1 else background[b]

            def render(k_cap, tile_hint):
                return _forward(view, view_needs, *params, cameras[2 * b], cameras[2 * b + 1], image_size, depth_range,
                                spec["config"], spec["render_depth"], spec["use_depth16"], spec["render_median"], None,
                                None, holder, "dense", "replicated", None, True, key, k_cap, tile_hint, colour,
                                spec["differentiable_weight"])
            outs.extend(_at_capacity(render, key))
            saved.extend(view.saved_tensors[5:])  # the contiguous camera matrices, the workspace
            views.append(view)
        frames = [(view.saved_tensors[7], view.meta["frame"][1], view.meta["V"]) for view in views]
        total = sum(V for _, _, V in frames)
        union = torch.empty((min(n, total),), dtype=torch.int64, device=dev)
        U = 0
        if total > 0:
            need = lib.gs_views_union_scratch_bytes(n)
            scratch = nv.scratch(need, dev)
            count = torch.empty((1,), dtype=torch.int32, device=dev)
            tables = (ctypes.c_void_p * len(frames))(*[ws.data_ptr() + L.slot_of for ws, L, _ in frames])
            nv.check(lib.gs_views_union(n, len(frames), tables, nv.ptr(union), nv.ptr(count), nv.ptr(scratch), need,
                                        nv.stream()), "gs_views_union")
            U = int(count.item())  # the one host read of the batch
        union = union[:U]
        visibility = _empty(dev, (0,))
        if spec["config"].compute_visibility:
            visibility = torch.empty((U,), dtype=torch.float32, device=dev)
            if U > 0:
                seen = [(ws, L, _carve(ws.view(torch.float32), L.visibility, (V,)), V, 1) for ws, L, V in frames]
                nv.check(lib.gs_views_sum_rows(U, nv.ptr(union), len(seen), _view_tables(seen), 1, nv.ptr(visibility),
                                               nv.stream()), "gs_views_sum_rows")
        for view in views:
            view.saved_tensors = ()
        ctx.views, ctx.spec = views, spec
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*params, union, *saved)
        ctx.mark_non_differentiable(*(t for view in views for t in view.non_differentiable), union, visibility)
        return (*outs, union, visibility)

    @staticmethod
    @nv.on_tensor_device
    def backward(ctx, *grads):
        saved = ctx.saved_tensors
        params, union = saved[:5], saved[5]
        views, needs = ctx.views, ctx.needs_input_grad
        dev, U = union.device, union.shape[0]
        need_background = needs[_VIEWS_CAMERAS - 1]
        camera_grads, background_grads = [None] * (2 * len(views)), [None] * len(views)
        done = []  # (workspace, layout, the five compact pieces, V) of the views that received a gradient, in view order
        for b, view in enumerate(views):
            g_image, g_alpha, g_points, g_depth, _, _, _, g_img_depth, g_img_var, _ = \
                grads[_VIEW_OUTPUTS * b:_VIEW_OUTPUTS * (b + 1)]
            if all(g is None for g in (g_image, g_alpha, g_points, g_depth, g_img_depth, g_img_var)):
                continue  # left out of the loss
            view.saved_tensors = (*params, *saved[6 + 3 * b:9 + 3 * b])
            rows, camera_grads[2 * b], camera_grads[2 * b + 1] = _backward_rows(view, g_image, g_points, g_depth,
                                                                                g_img_depth, g_img_var, g_alpha)
            if need_background:
                background_grads[b] = _background_grad(view, g_image)
            done.append((view.saved_tensors[7], view.meta["frame"][1], rows, view.meta["V"]))
            view.saved_tensors = ()
        # the merged rows: one allocation, the pieces on 256-byte boundaries like the frames' own
        widths = [t.numel() // t.shape[0] for t in params]
        starts, at = [], 0
        for width in widths:
            starts.append(at)
            at += -(-U * width // 64) * 64
        flat = torch.empty((at,), dtype=torch.float32, device=dev)
        merged = [flat.as_strided((U, *t.shape[1:]), t.stride(), start) for t, start in zip(params, starts)]
        if U > 0:
            lib = nv.lib()
            for k, width in enumerate(widths):
                entries = [(ws, L, rows[k], V, width) for ws, L, rows, V in done]
                nv.check(lib.gs_views_sum_rows(U, nv.ptr(union), len(entries), _view_tables(entries), width,
                                               nv.ptr(merged[k]), nv.stream()), "gs_views_sum_rows")
        if ctx.spec["sparse_grad"]:
            idx = union.clone().view(1, U)  # fresh and shared by the five: .grad keeps neither a workspace nor the node
            _register_sparse_indexes(idx)
            d_params = [torch.sparse_coo_tensor(idx, r, t.shape, is_coalesced=True) for r, t in zip(merged, params)]
        else:
            d_params = [torch.zeros_like(t).index_copy_(0, union, r) for r, t in zip(merged, params)]
        d_background = None
        if need_background:
            C = params[4].shape[1]
            parts = [torch.zeros((C,), dtype=torch.float32, device=dev) if g is None else g for g in background_grads]
            d_background = torch.stack(parts)
            if ctx.spec["background_dim"] == 1:
                d_background = d_background.sum(0)
        return (*d_params, None, d_background, *camera_grads)


def render_views_fused(gaussians, cameras, config: RasterConfig, render_depth: bool, use_depth16: bool,
                       render_median_depth: bool, sparse_grad: bool, background, differentiable_weight: bool):
    """(the views' Renderings, the union of their points_in_view, its summed visibility or None): see
    renderer.render_views and _ViewsRender"""
    from .renderer import Rendering
    params = (gaussians.position.contiguous(), gaussians.log_scaling.contiguous(), gaussians.rotation.contiguous(),
              gaussians.alpha_logit.contiguous(), gaussians.feature.contiguous())
    n = params[0].shape[0]
    frames, matrices = [], []
    for cam in cameras:
        size = cam.image_size
        key = (n, int(size[0]), int(size[1]), None, config.tile_size, bool(use_depth16))
        frames.append((size, cam.depth_range, {}, key))
        matrices += [cam.T_camera_world, cam.projection]
    spec = dict(frames=frames, config=config, render_depth=render_depth, use_depth16=use_depth16,
                render_median=render_median_depth, differentiable_weight=bool(differentiable_weight),
                sparse_grad=bool(sparse_grad), background_dim=0 if background is None else background.dim())
    outs = _ViewsRender.apply(*params, spec, background, *matrices)
    renderings = []
    for b, cam in enumerate(cameras):
        image, alpha, g2d, depths, indexes, vis, heur, img_depth, img_var, median = \
            outs[_VIEW_OUTPUTS * b:_VIEW_OUTPUTS * (b + 1)]
        frames[b][2]["gaussians2d"] = weakref.ref(g2d)
        indexes._gs_unique = True
        renderings.append(Rendering(
            image=image, image_weight=alpha, depth=img_depth if render_depth else None,
            depth_var=img_var if render_depth else None, median_depth=median if render_median_depth else None,
            camera=cam, config=config, point_visibility=vis if config.compute_visibility else None,
            point_heuristic=heur if config.compute_point_heuristic else None, points_in_view=indexes,
            point_depth=depths, gaussians2d=g2d))
    union, visibility = outs[-2], outs[-1]
    union._gs_unique = True
    return renderings, union, visibility if config.compute_visibility else None


def fused_supported(gaussians, camera_params, use_sh: bool, render_median_depth: bool) -> bool:
    """The fused node covers SH colours (N, C <= 8, D) and plain features (N, C <= 30), with or without the depth
    and median-depth images, camera gradients included.  What is left -- an empty scene, wider features -- runs the
    composed operators."""
    f = gaussians.feature
    if gaussians.position.shape[0] == 0 or not f.is_cuda or f.dtype != torch.float32:
        return False
    if use_sh:
        return f.ndim == 3 and f.shape[1] <= 8
    return f.ndim == 2 and 1 <= f.shape[1] <= 30


def _capacity(hint):
    """(k_cap, tile_hint) of a frame call: capacities rounded up to a few classes so that the cached frame descriptors
    and workspace layouts are reused from frame to frame"""
    k_cap = -(-(int(hint[0] * 1.25) + 4096) // 65536) * 65536
    tile_hint = next((c for c in (256, 512, 1024, 2048) if hint[1] <= c), 4096)
    return k_cap, tile_hint


def _at_capacity(render, key):
    """render(k_cap, tile_hint) at the capacity class of the shape `key` (seen for the first time: the smallest class); a
    frame with more overlaps than that is run once more, sized for the K its first attempt recorded"""
    outs = None
    try:
        outs = render(*_capacity(_K_HINT.get(key, (0, 0))))
    except _Overflow:  # more overlaps than the capacity: K is recorded now
        pass
    if outs is None:
        # run again outside the except block, whose traceback still holds the failed attempt's workspace; the mapper
        # is deterministic, so the same frame at a capacity of at least its K cannot overflow again
        try:
            outs = render(*_capacity(_K_HINT[key]))
        except _Overflow:
            raise RuntimeError(f"render_gaussians: the re-run of an overflowing frame overflowed again (hint "
                               f"{_K_HINT[key]})") from None
    return outs


def render_fused(gaussians, camera_params, config: RasterConfig, render_depth: bool, use_depth16: bool,
                 shard=None, group=None, render_median_depth: bool = False, exchange: str = "dense",
                 grad_mode: str = "replicated", owned=None, owned_range=None, sparse_grad: bool = False,
                 background=None, differentiable_weight: bool = False):
    """shard (parallel.RowShard): render only the tile rows this rank owns; the images then hold those pixel rows,
    everything per-Gaussian (`gaussians2d` included) stays in full-image coordinates.
    See parallel.render_gaussians_sharded.
    sparse_grad: the five Gaussian parameters receive sparse COO gradients over points_in_view (renderer.py).
    background, differentiable_weight: see renderer.render_gaussians; not with a shard."""
    import weakref

    from .renderer import Rendering
    if shard is not None and (background is not None or differentiable_weight):
        raise NotImplementedError("render_fused: a sharded frame has neither a background nor a differentiable "
                                  "image_weight (parallel.render_gaussians_sharded does not take the arguments)")
    holder = {}
    args = (gaussians.position.contiguous(), gaussians.log_scaling.contiguous(), gaussians.rotation.contiguous(),
            gaussians.alpha_logit.contiguous(), gaussians.feature.contiguous(), camera_params.T_camera_world,
            camera_params.projection, camera_params.image_size, camera_params.depth_range, config, render_depth,
            use_depth16, render_median_depth, shard, group, holder, exchange, grad_mode, owned_range, bool(sparse_grad))
    size = camera_params.image_size
    key = (args[0].shape[0], int(size[0]), int(size[1]), shard, config.tile_size, bool(use_depth16))
    if owned is not None:
        # grad_mode "sharded": gradients flow to the rank's own rows (range-shaped leaf tensors), see _OwnedRender
        own = (owned.position.contiguous(), owned.log_scaling.contiguous(), owned.rotation.contiguous(),
               owned.alpha_logit.contiguous(), owned.feature.contiguous())
        full = tuple(t.detach() for t in args[:7])

        def render(*sizes):
            return _OwnedRender.apply(*own, full, (*args[7:], key, *sizes))
    else:
        def render(*sizes):
            return _FrameRender.apply(*args, key, *sizes, background, bool(differentiable_weight))
    outs = _at_capacity(render, key)
    image, alpha, g2d, depths, indexes, vis, heur, img_depth, img_var, median = outs
    holder["gaussians2d"] = weakref.ref(g2d)
    indexes._gs_unique = True
    if not render_depth:
        img_depth = img_var = None
    rendering = Rendering(image=image, image_weight=alpha, depth=img_depth, depth_var=img_var,
                          median_depth=median if render_median_depth else None, camera=camera_params, config=config,
                          point_visibility=vis if config.compute_visibility else None,
                          point_heuristic=heur if config.compute_point_heuristic else None,
                          points_in_view=indexes, point_depth=depths, gaussians2d=g2d)
    if shard is not None:  # how many splats can reach this rank's rows (= its list in a sparse exchange)
        object.__setattr__(rendering, "touched_count", holder.get("touched_count"))
    return rendering
