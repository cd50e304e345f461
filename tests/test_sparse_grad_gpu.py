"""render_gaussians(sparse_grad=True): the backward leaves torch.sparse_coo gradients over points_in_view, produced by
row-compact adjoints (gs_project_bwd_rows, gs_sh_bwd_rows, gs_feature_gather_bwd_rows through gs_frame_bwd_rows), and the
optimizers step from them (gs_optim_step_rows).  Everything is compared with the dense path on the same inputs.

The scene is half in view: a benchmark scene plus a copy mirrored behind the camera, rows shuffled, so that the visible
set is neither everything nor a prefix of the rows."""
import ctypes

import pytest
import torch

import config_cases as cc
import parity_util as pu
import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import RasterConfig, _native as nv, scenes

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PARAMS = ("position", "log_scaling", "rotation", "alpha_logit", "feature")
ROW_FLOATS = 16  # the row stride of the rasterizer's gradient rows for up to 7 features


def half_in_view(n, size, sh_degree, seed):
    """(2 n Gaussians of which n are behind the camera, camera)"""
    g, cam = scenes.benchmark_scene(n, size, sh_degree=sh_degree, seed=seed)
    behind = g.replace(position=g.position * torch.tensor([1.0, 1.0, -1.0]))
    both = g.concat(behind)
    perm = torch.randperm(2 * n, generator=torch.Generator().manual_seed(seed + 100))
    return both[perm].contiguous(), cam


def check_half_in_view(indexes, total):
    V = int(indexes.shape[0])
    assert 0 < V <= total // 2, f"{V} of {total} rows in view: the scene is not half in view"
    assert int(indexes[-1]) >= V, "the visible set is a prefix of the rows"
    assert bool((indexes[1:] > indexes[:-1]).all()), "points_in_view is not ascending"
    return V


def off(t, floats):
    return ctypes.c_void_p(t.data_ptr() + 4 * floats)


def visible_set(g, cam, cfg):
    from taichi_gaussian_rasterizer_amd.perspective.projection import project_with_ndc
    with torch.no_grad():
        _, _, indexes, _ = project_with_ndc(*g.shape_tensors(), cam.T_camera_world, cam.projection, cam.image_size,
                                            cam.depth_range, cfg)
    n = g.position.shape[0]
    slot_of = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    slot_of[indexes] = torch.arange(indexes.shape[0], dtype=torch.int32, device=DEV)
    return indexes.contiguous(), slot_of


# ------------------------------------------------------------------------------------------------- 1. operators
def test_project_bwd_rows_matches_dense_rows():
    n, size = 4000, (224, 160)
    cfg = RasterConfig()
    g, cam = half_in_view(n, size, 0, 21)
    g, cam = g.to(DEV), cam.to(device=DEV)
    N = 2 * n
    indexes, slot_of = visible_set(g, cam, cfg)
    V = check_half_in_view(indexes, N)
    rows = torch.randn(V, ROW_FLOATS, generator=torch.Generator().manual_seed(5)).to(DEV)
    lib, c = nv.lib(), nv.make_config(cfg)
    T, proj = cam.T_camera_world.contiguous(), cam.projection.contiguous()
    shapes = ((3,), (3,), (4,), (1,))
    dense = [torch.full((N, *s), 7.0, device=DEV) for s in shapes]
    compact = [torch.full((V, *s), 7.0, device=DEV) for s in shapes]
    cams = [torch.empty(4, 4, device=DEV), torch.empty(4, device=DEV), torch.empty(4, 4, device=DEV),
            torch.empty(4, device=DEV)]
    nb = lib.gs_project_bwd_scratch_bytes(N)
    scratch = torch.empty(nb, dtype=torch.uint8, device=DEV)
    # the upstream gradients as the frame hands them over: splat columns 0..6, z and z^2 columns 7 and 8 of the rows
    nv.check(lib.gs_project_bwd(N, V, *map(nv.ptr, g.shape_tensors()), nv.ptr(T), nv.ptr(proj), size[0], size[1], c,
                                nv.ptr(slot_of), nv.ptr(rows), ROW_FLOATS, off(rows, 7), off(rows, 8), ROW_FLOATS,
                                *map(nv.ptr, dense), nv.ptr(cams[0]), nv.ptr(cams[1]), nv.ptr(scratch), nb,
                                nv.stream()), "gs_project_bwd")
    nbr = lib.gs_project_bwd_rows_scratch_bytes(V)
    scratch_r = torch.empty(nbr, dtype=torch.uint8, device=DEV)
    nv.check(lib.gs_project_bwd_rows(N, V, *map(nv.ptr, g.shape_tensors()), nv.ptr(T), nv.ptr(proj), size[0], size[1],
                                     c, nv.ptr(indexes), nv.ptr(rows), ROW_FLOATS, off(rows, 7), off(rows, 8),
                                     ROW_FLOATS, *map(nv.ptr, compact), nv.ptr(cams[2]), nv.ptr(cams[3]),
                                     nv.ptr(scratch_r), nbr, nv.stream()), "gs_project_bwd_rows")
    culled = slot_of < 0
    for name, d, r in zip(PARAMS, dense, compact):
        assert torch.equal(r, d[indexes]), f"{name}: compact rows differ from the dense kernel's"
        assert float(d[culled].abs().max()) == 0.0, f"{name}: dense rows of culled Gaussians are not zero"
        assert float(r.abs().max()) > 0.0
    pu.assert_grad_close(cams[2], cams[0], "d_T_camera_world", tol=1e-3)
    pu.assert_grad_close(cams[3], cams[1], "d_projection", tol=1e-3)
    # without camera outputs (the other instantiation), and without scratch
    again = [torch.empty_like(r) for r in compact]
    nv.check(lib.gs_project_bwd_rows(N, V, *map(nv.ptr, g.shape_tensors()), nv.ptr(T), nv.ptr(proj), size[0], size[1],
                                     c, nv.ptr(indexes), nv.ptr(rows), ROW_FLOATS, off(rows, 7), off(rows, 8),
                                     ROW_FLOATS, *map(nv.ptr, again), None, None, None, 0, nv.stream()),
             "gs_project_bwd_rows")
    dense2 = [torch.empty_like(d) for d in dense]
    nv.check(lib.gs_project_bwd(N, V, *map(nv.ptr, g.shape_tensors()), nv.ptr(T), nv.ptr(proj), size[0], size[1], c,
                                nv.ptr(slot_of), nv.ptr(rows), ROW_FLOATS, off(rows, 7), off(rows, 8), ROW_FLOATS,
                                *map(nv.ptr, dense2), None, None, None, 0, nv.stream()), "gs_project_bwd")
    for name, d, r in zip(PARAMS, dense2, again):
        assert torch.equal(r, d[indexes]), f"{name} (no camera gradients)"


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_sh_bwd_rows_matches_dense_rows(degree, channels, masked):
    n, size = 3000, (224, 160)
    cfg = RasterConfig()
    g, cam = half_in_view(n, size, degree, 23)
    N, D = 2 * n, (degree + 1) ** 2
    gen = torch.Generator().manual_seed(9)
    # coefficients large enough that the clamp is active for part of the rows
    feature = (g.feature[:, :channels] + 0.6 * torch.randn(N, channels, D, generator=gen)).contiguous()
    g, cam = g.replace(feature=feature).to(DEV), cam.to(device=DEV)
    indexes, slot_of = visible_set(g, cam, cfg)
    V = check_half_in_view(indexes, N)
    rows = torch.randn(V, ROW_FLOATS, generator=gen).to(DEV)
    centre = cam.camera_position.contiguous()
    with torch.no_grad():
        colours = gs.evaluate_sh_at(g.feature, g.position, indexes, centre).contiguous()
    clamped = (colours <= 0) | (colours >= 1)
    assert 0 < int(clamped.sum()) < clamped.numel()
    lib = nv.lib()
    dense = torch.full((N, channels, D), 7.0, device=DEV)
    compact = torch.full((V, channels, D), 7.0, device=DEV)
    if masked:   # the clamp mask comes from the forward's output; no view-direction gradient
        extra_d = extra_r = (None, None)
        fwd = (nv.ptr(colours), channels)
    else:        # the coefficients are re-read; with d_positions and d_camera_pos
        dpos_d, dpos_r = torch.full((N, 3), 7.0, device=DEV), torch.full((V, 3), 7.0, device=DEV)
        dcam_d, dcam_r = torch.full((3,), 7.0, device=DEV), torch.full((3,), 7.0, device=DEV)
        extra_d, extra_r = (nv.ptr(dpos_d), nv.ptr(dcam_d)), (nv.ptr(dpos_r), nv.ptr(dcam_r))
        fwd = (None, 0)
    nv.check(lib.gs_sh_bwd(N, V, channels, degree, nv.ptr(g.feature), nv.ptr(g.position), nv.ptr(indexes), 1,
                           nv.ptr(slot_of), nv.ptr(centre), off(rows, 7), ROW_FLOATS, *fwd, nv.ptr(dense), *extra_d,
                           nv.stream()), "gs_sh_bwd")
    nv.check(lib.gs_sh_bwd_rows(N, V, channels, degree, nv.ptr(g.feature), nv.ptr(g.position), nv.ptr(indexes),
                                nv.ptr(centre), off(rows, 7), ROW_FLOATS, *fwd, nv.ptr(compact), *extra_r,
                                nv.stream()), "gs_sh_bwd_rows")
    assert torch.equal(compact, dense[indexes])
    assert float(dense[slot_of < 0].abs().max()) == 0.0
    assert float(compact.abs().max()) > 0.0
    if masked:  # the clamped channels got no gradient
        assert float(compact[clamped].abs().max()) == 0.0
    else:
        assert torch.equal(dpos_r, dpos_d[indexes])
        assert float(dpos_d[slot_of < 0].abs().max()) == 0.0
        if degree >= 1:
            pu.assert_grad_close(dcam_r, dcam_d, "d_camera_pos", tol=1e-3)
        else:
            assert float(dcam_r.abs().max()) == 0.0 and float(dcam_d.abs().max()) == 0.0


@pytest.mark.parametrize("channels", [1, 6])
def test_feature_gather_bwd_rows_matches_dense_rows(channels):
    n, size = 3000, (224, 160)
    cfg = RasterConfig()
    g, cam = half_in_view(n, size, 0, 25)
    g, cam = g.to(DEV), cam.to(device=DEV)
    N = 2 * n
    indexes, slot_of = visible_set(g, cam, cfg)
    V = check_half_in_view(indexes, N)
    rows = torch.randn(V, ROW_FLOATS, generator=torch.Generator().manual_seed(4)).to(DEV)
    lib = nv.lib()
    dense = torch.full((N, channels), 7.0, device=DEV)
    compact = torch.full((V, channels), 7.0, device=DEV)
    nv.check(lib.gs_feature_gather_bwd(N, channels, nv.ptr(slot_of), off(rows, 9), ROW_FLOATS, nv.ptr(dense),
                                       nv.stream()), "gs_feature_gather_bwd")
    nv.check(lib.gs_feature_gather_bwd_rows(V, channels, off(rows, 9), ROW_FLOATS, nv.ptr(compact), nv.stream()),
             "gs_feature_gather_bwd_rows")
    assert torch.equal(compact, dense[indexes]) and torch.equal(compact, rows[:, 9:9 + channels])
    assert float(dense[slot_of < 0].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------- 2. frames
def _frame_case(case):
    size, n = (224, 160), 5000
    if case == "sh3":
        g, cam = half_in_view(n, size, 3, 31)
        g = g.replace(feature=g.feature + 0.3 * torch.randn(g.feature.shape, generator=torch.Generator().manual_seed(2)))
        kw = dict(use_sh=True)
        cfg = RasterConfig(compute_visibility=True, compute_point_heuristic=True)
    elif case == "plain6_depth":
        g, cam = half_in_view(n, size, 0, 33)
        g = g.replace(feature=torch.rand(2 * n, 6, generator=torch.Generator().manual_seed(8)))
        kw = dict(use_sh=False, render_depth=True)
        cfg = RasterConfig()
    else:  # "camera": pose refinement through SH colours, both camera matrices require gradients
        g, cam = half_in_view(n, size, 3, 35)
        tilt = torch.eye(4)
        tilt[:3, :3] = torch.linalg.qr(torch.eye(3) + 0.05 * torch.randn(3, 3,
                                                                          generator=torch.Generator().manual_seed(4))).Q
        tilt[:3, 3] = torch.tensor([0.02, -0.01, 0.03])
        cam = cam.transformed(tilt)
        kw = dict(use_sh=True)
        cfg = RasterConfig()
    return g, cam, cfg, kw


def _loss(r, gi, kw):
    loss = (r.image * gi).sum()
    if kw.get("render_depth"):
        loss = loss + r.depth.sum() + 0.1 * r.depth_var.sum()
    return loss


VALUE_TAIL = dict(position=(3,), log_scaling=(3,), rotation=(4,), alpha_logit=(1,))


@pytest.mark.parametrize("case", ["sh3", "plain6_depth", "camera"])
def test_frame_sparse_gradients_match_dense(case, frame_path):
    _frame_sparse_gradients_match_dense(case, *_frame_case(case))


@pytest.mark.parametrize("fid", ["frame_a", "frame_b"])
def test_frame_sparse_gradients_match_dense_at_other_settings(fid, frame_path):
    """gs_frame_bwd_rows at tile sizes 8 and 32 with every threshold, clamp, margin and blur away from its default, on
    the settings sweep's scene made half in view, with depth outputs"""
    s = cc.FRAME_SCENE
    g, camera = half_in_view(s["n"], s["size"], s["sh_degree"], s["seed"])
    _frame_sparse_gradients_match_dense(fid, g, camera, cc.frame_config(fid), dict(use_sh=True, render_depth=True))


def _frame_sparse_gradients_match_dense(case, g, camera, cfg, kw):
    N = g.position.shape[0]
    C = g.feature.shape[1]
    gi = torch.rand(camera.image_size[1], camera.image_size[0], C, generator=torch.Generator().manual_seed(3)).to(DEV)
    runs = {}
    for sparse in (False, True):
        cam = camera.to(device=DEV)
        if case == "camera":
            cam.T_camera_world.requires_grad_(True)
            cam.projection.requires_grad_(True)
        a = g.to(DEV).requires_grad_(True)
        r = gs.render_gaussians(a, cam, cfg, sparse_grad=sparse, **kw)
        r.gaussians2d.retain_grad()
        _loss(r, gi, kw).backward()
        runs[sparse] = (a, r, cam)
    (ad, rd, cd), (as_, rs, cs) = runs[False], runs[True]
    assert torch.equal(rd.image, rs.image) and torch.equal(rd.points_in_view, rs.points_in_view)
    V = check_half_in_view(rs.points_in_view, N)
    if kw.get("render_depth"):
        assert torch.equal(rd.depth, rs.depth) and torch.equal(rd.depth_var, rs.depth_var)
    shared = None
    for name in PARAMS:
        dense, sp = getattr(ad, name).grad, getattr(as_, name).grad
        assert not dense.is_sparse and sp.is_sparse, name
        assert sp.shape == dense.shape and sp._nnz() == V
        idx = sp._indices()
        assert idx.shape == (1, V) and idx.dtype == torch.int64 and torch.equal(idx[0], rs.points_in_view)
        # one fresh index tensor for the five gradients, and not a view of the frame's workspace
        shared = idx.data_ptr() if shared is None else shared
        assert idx.data_ptr() == shared and idx.data_ptr() != rs.points_in_view.data_ptr()
        tail = VALUE_TAIL.get(name, tuple(g.feature.shape[1:]))
        assert tuple(sp._values().shape) == (V, *tail), name
        pu.assert_grad_close(sp.to_dense(), dense, f"{case}: grad {name}", tol=1e-3)
        outside = torch.ones(N, dtype=torch.bool, device=DEV)
        outside[rs.points_in_view] = False
        assert float(dense[outside].abs().max()) == 0.0
    pu.assert_grad_close(rs.gaussians2d.grad, rd.gaussians2d.grad, f"{case}: gaussians2d.grad", tol=1e-3)
    if cfg.compute_point_heuristic:
        pu.assert_grad_close(rs.point_heuristic, rd.point_heuristic, f"{case}: point_heuristic", tol=1e-3)
    if case == "camera":
        for t_d, t_s, name in ((cd.T_camera_world, cs.T_camera_world, "T_camera_world"),
                               (cd.projection, cs.projection, "projection")):
            assert not t_s.grad.is_sparse and t_s.grad.shape == t_d.grad.shape
            pu.assert_grad_close(t_s.grad, t_d.grad, f"grad {name}", tol=1e-3)


# ------------------------------------------------------------------------------------------------- 3. accumulation
def test_two_backward_passes_and_a_dense_gradient_already_present(frame_path):
    g, camera, cfg, kw = _frame_case("sh3")
    cam = camera.to(device=DEV)
    gi = torch.rand(camera.image_size[1], camera.image_size[0], 3, generator=torch.Generator().manual_seed(3)).to(DEV)

    def once(backwards, preset=None):
        a = g.to(DEV).requires_grad_(True)
        if preset is not None:
            for name in PARAMS:
                getattr(a, name).grad = preset[name].clone()
        r = gs.render_gaussians(a, cam, cfg, sparse_grad=True, **kw)
        loss = _loss(r, gi, kw)
        for k in range(backwards):
            loss.backward(retain_graph=k + 1 < backwards)
        return a

    one, two = once(1), once(2)
    for name in PARAMS:
        g1, g2 = getattr(one, name).grad, getattr(two, name).grad
        assert g1.is_sparse and g2.is_sparse
        pu.assert_grad_close(g2.to_dense(), 2.0 * g1.to_dense(), f"two backward passes: grad {name}", tol=1e-3)
    gen = torch.Generator().manual_seed(6)
    preset = {name: torch.randn(getattr(g, name).shape, generator=gen).to(DEV) for name in PARAMS}
    mixed = once(1, preset)
    for name in PARAMS:
        got = getattr(mixed, name).grad
        assert not got.is_sparse, f"{name}: dense + sparse must be dense"
        pu.assert_grad_close(got, preset[name] + getattr(one, name).grad.to_dense(), f"dense + sparse: grad {name}",
                             tol=1e-3)


def test_nothing_in_view_gives_empty_sparse_gradients(frame_path):
    n, size = 2000, (160, 128)
    g, cam = scenes.benchmark_scene(n, size, sh_degree=3, seed=41)
    g = g.replace(position=g.position * torch.tensor([1.0, 1.0, -1.0]))   # everything behind the camera
    a, cam = g.to(DEV).requires_grad_(True), cam.to(device=DEV)
    r = gs.render_gaussians(a, cam, RasterConfig(compute_visibility=True, compute_point_heuristic=True), use_sh=True,
                            sparse_grad=True)
    assert r.points_in_view.shape[0] == 0
    (r.image.sum() + r.gaussians2d.sum()).backward()
    torch.cuda.synchronize()
    for name in PARAMS:
        grad = getattr(a, name).grad
        assert grad.is_sparse and grad._nnz() == 0 and grad.shape == getattr(a, name).shape
        assert float(grad.to_dense().abs().max()) == 0.0


def test_unsupported_frames_raise_before_any_launch():
    n, size = 500, (64, 48)
    g, cam = scenes.benchmark_scene(n, size, sh_degree=0, seed=43)
    g = g.replace(feature=torch.rand(n, 31)).to(DEV).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="sparse"):
        gs.render_gaussians(g, cam.to(device=DEV), RasterConfig(), use_sh=False, sparse_grad=True)
    # the same frame renders through the composed operators without the switch
    r = gs.render_gaussians(g, cam.to(device=DEV), RasterConfig(), use_sh=False)
    assert r.image.shape[-1] == 31


# ------------------------------------------------------------------------------------------------- 4. optimizers
OPTIMIZERS = {"FractionalAdam": False, "FractionalLaProp": False, "VisibilityAwareAdam": True,
              "VisibilityAwareLaProp": True}


def _optimizer_pair(name, n, seed):
    from test_optim_gpu import _groups
    from taichi_gaussian_rasterizer_amd import optim
    params, types = _groups(n, seed)
    lrs = dict(position=0.01, log_scaling=0.02, rotation=0.005, alpha_logit=0.05, feature=0.03)
    g = torch.Generator().manual_seed(7)
    mask_lr = torch.rand(3, 4, generator=g)
    point_lr = torch.rand(n, generator=g) + 0.5
    out = []
    for _ in range(2):
        dev_params = {k: torch.nn.Parameter(v.clone().to(DEV)) for k, v in params.items()}
        groups = [dict(params=[dev_params[k]], name=k, type=types[k], lr=lrs[k],
                       mask_lr=mask_lr.to(DEV) if k == "feature" else None,
                       point_lr=point_lr.to(DEV) if k == "position" else None) for k in params]
        out.append((dev_params, getattr(optim, name)(groups, betas=(0.9, 0.999))))
    return out, types, g


def _assert_same_training_state(dense, sparse, types, what):
    (pd, od), (ps, os_) = dense, sparse
    for k, kind in types.items():
        sd, ss = od.state[pd[k]], os_.state[ps[k]]
        if kind == "local_vector":  # the gradient takes another route into the local frame: the existing file's bar
            assert torch.allclose(ps[k], pd[k], rtol=2e-5, atol=1e-6), (what, k, (ps[k] - pd[k]).abs().max())
            for key in ("v", "m"):
                assert torch.allclose(ss[key], sd[key], rtol=2e-5, atol=1e-6), (what, k, key)
        else:  # the same arithmetic on the same numbers
            assert torch.equal(ps[k], pd[k]), (what, k, (ps[k] - pd[k]).abs().max())
            for key in ("v", "m"):
                assert torch.equal(ss[key], sd[key]), (what, k, key)
    first = next(iter(types))
    for key in ("total_weight", "running_vis"):
        if key in od.state[pd[first]]:
            assert torch.equal(os_.state[ps[first]][key], od.state[pd[first]][key]), (what, key)


@pytest.mark.parametrize("case", ["same", "subset", "outside"])
@pytest.mark.parametrize("name", sorted(OPTIMIZERS))
def test_optimizers_step_from_sparse_gradients(name, case):
    n = 5000
    (dense, sparse), types, g = _optimizer_pair(name, n, 3)
    visibility = OPTIMIZERS[name]
    initial = dense[0]["feature"].detach().clone()
    for step in range(6):
        S = torch.randperm(n, generator=g)[: n // 2].sort().values
        if case == "same":
            idx = S
        elif case == "subset":
            idx = S[torch.rand(S.shape[0], generator=g) < 0.6]
            assert 0 < idx.shape[0] < S.shape[0]
        else:
            member = torch.zeros(n, dtype=torch.bool)
            member[S] = True
            idx = torch.nonzero((torch.rand(n, generator=g) < 0.4)).flatten()
            assert bool(member[idx].any()) and not bool(member[idx].all())
        w = torch.rand(idx.shape[0], generator=g) * (0.9 if visibility else 1.5) + 0.05
        q = torch.linalg.qr(torch.randn(idx.shape[0], 3, 3, generator=g)).Q * \
            (0.5 + torch.rand(idx.shape[0], 1, 1, generator=g))
        S_dev = S.to(DEV)
        for k, p in dense[0].items():
            rows = torch.randn((S.shape[0], *p.shape[1:]), generator=g).to(DEV)
            full = torch.zeros_like(p)
            full[S_dev] = rows
            p.grad = full
            sparse[0][k].grad = torch.sparse_coo_tensor(S_dev[None], rows, p.shape, is_coalesced=True)
        for _, opt in (dense, sparse):
            opt.step(idx.to(DEV), w.to(DEV), basis=q.to(DEV))
    assert all(p.grad.is_sparse for p in sparse[0].values())
    _assert_same_training_state(dense, sparse, types, f"{name}/{case}")
    assert not torch.equal(dense[0]["feature"].detach(), initial)


@pytest.mark.parametrize("name", sorted(OPTIMIZERS))
def test_uncoalesced_sparse_gradient_steps_like_its_dense_sum(name):
    """the slow path: a sparse gradient that is not a frame's (two concatenated halves, one row listed twice) goes
    through coalesce()"""
    n = 3000
    (dense, sparse), types, g = _optimizer_pair(name, n, 5)
    S = torch.randperm(n, generator=g)[: n // 2].sort().values
    half = S.shape[0] // 2
    listed = torch.cat([S[half:], S[:half], S[:1]]).to(DEV)
    idx = S[::2]
    w = torch.rand(idx.shape[0], generator=g) * 0.9 + 0.05
    q = torch.linalg.qr(torch.randn(idx.shape[0], 3, 3, generator=g)).Q
    for k, p in dense[0].items():
        rows = torch.randn((listed.shape[0], *p.shape[1:]), generator=g).to(DEV)
        grad = torch.sparse_coo_tensor(listed[None], rows, p.shape)
        assert not grad.is_coalesced()
        sparse[0][k].grad = grad
        p.grad = grad.to_dense()
    for _, opt in (dense, sparse):
        opt.step(idx.to(DEV), w.to(DEV), basis=q.to(DEV))
    _assert_same_training_state(dense, sparse, types, name)


def test_finite_check_reads_the_values_of_a_sparse_gradient():
    from taichi_gaussian_rasterizer_amd.torch_lib.util import count_nonfinite
    p = torch.nn.Parameter(torch.zeros(10, 3, device=DEV))
    values = torch.ones(2, 3, device=DEV)
    values[1, 2] = float("nan")
    p.grad = torch.sparse_coo_tensor(torch.tensor([[2, 5]], device=DEV), values, p.shape, is_coalesced=True)
    assert count_nonfinite(p, "p") == {"p.grad": 1}


def test_step_from_a_frame_gradient_equals_the_step_from_its_dense_form(frame_path):
    """the optimizer's fast path: the gradient a frame left on the parameters (recognised by the address of its index
    list, is_coalesced dropped by autograd) and a step over a subset of points_in_view.  A second set of parameters
    holds the same gradient as a dense tensor; parameters and state are then the same bits"""
    from taichi_gaussian_rasterizer_amd.fused import is_frame_sparse_grad
    from taichi_gaussian_rasterizer_amd.optim import VisibilityAwareAdam
    n, size = 6000, (256, 192)
    g, cam = half_in_view(n, size, 3, 61)
    N = 2 * n
    cam = cam.to(device=DEV)
    kinds = (("position", 1e-3, "vector"), ("log_scaling", 1e-2, "vector"), ("rotation", 1e-2, "vector"),
             ("alpha_logit", 1e-1, "scalar"), ("feature", 1e-2, "scalar"))
    types = {k: t for k, _, t in kinds}
    sets = []
    for _ in range(2):
        params = {k: torch.nn.Parameter(v.clone().to(DEV)) for k, v in g.items()}
        sets.append((params, VisibilityAwareAdam([dict(params=[params[k]], name=k, lr=lr, type=t)
                                                  for k, lr, t in kinds])))
    (pd, od), (ps, os_) = sets
    cfg = RasterConfig(compute_visibility=True)
    target = torch.rand(size[1], size[0], 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    for step in range(3):
        os_.zero_grad()
        r = gs.render_gaussians(type(g)(**ps, batch_size=(N,)), cam, cfg, use_sh=True, sparse_grad=True)
        torch.nn.functional.l1_loss(r.image, target).backward()
        V = check_half_in_view(r.points_in_view, N)
        for k in ps:
            assert is_frame_sparse_grad(ps[k].grad) and not ps[k].grad.is_coalesced()
            pd[k].grad = ps[k].grad.to_dense()
        keep = r.point_visibility > 1e-8
        keep[::7] = False  # a strict subset whatever the visibilities are
        idx, w = r.points_in_view[keep], r.point_visibility[keep]
        assert 0 < idx.shape[0] < V
        od.step(idx, w)
        os_.step(idx, w)
        _assert_same_training_state((pd, od), (ps, os_), types, f"step {step}")
    assert not torch.equal(ps["feature"].detach(), g.feature.to(DEV))


# ------------------------------------------------------------------------------------------------- 5. training
def test_training_loop_on_sparse_gradients(frame_path):
    """tools/exp_train_host.py's loop, 20 iterations on the half-in-view scene"""
    from taichi_gaussian_rasterizer_amd.fused import is_frame_sparse_grad
    from taichi_gaussian_rasterizer_amd.optim import VisibilityAwareLaProp
    n, size = 10_000, (320, 240)
    g, cam = half_in_view(n, size, 3, 51)
    N = 2 * n
    cam = cam.to(device=DEV)
    start = {k: v.to(DEV) for k, v in g.items()}
    params = {k: torch.nn.Parameter(v.clone()) for k, v in start.items()}
    groups = [dict(params=[params[k]], name=k, lr=lr, type=t) for k, lr, t in
              (("position", 1e-4, "vector"), ("log_scaling", 1e-3, "vector"), ("rotation", 1e-3, "vector"),
               ("alpha_logit", 1e-2, "scalar"), ("feature", 1e-3, "scalar"))]
    opt = VisibilityAwareLaProp(groups)
    cfg = RasterConfig(compute_visibility=True, compute_point_heuristic=True)
    target = torch.rand(size[1], size[0], 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    seen = torch.zeros(N, dtype=torch.bool, device=DEV)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        gg = type(g)(**params, batch_size=(N,))
        r = gs.render_gaussians(gg, cam, cfg, use_sh=True, sparse_grad=True)
        loss = torch.nn.functional.l1_loss(r.image, target)
        loss.backward()
        assert all(p.grad.is_sparse and is_frame_sparse_grad(p.grad) for p in params.values())
        vis = r.point_visibility
        keep = vis > 1e-8
        idx, w = r.points_in_view[keep], vis[keep]
        seen[idx] = True
        opt.step(idx, w)
        losses.append(float(loss.detach()))
    check_half_in_view(r.points_in_view, N)
    assert 0 < int(seen.sum()) <= N // 2
    for k, p in params.items():
        assert bool(torch.isfinite(p).all()), k
        assert torch.equal(p.detach()[~seen], start[k][~seen]), f"{k}: a row that was never in view moved"
        assert not torch.equal(p.detach()[seen], start[k][seen]), f"{k}: nothing was trained"
    total_weight = opt.state[params["position"]]["total_weight"]
    assert float(total_weight[~seen].abs().max()) == 0.0 and float(total_weight[seen].min()) > 0.0
    assert losses[-1] < losses[0], losses
