"""Densification on the GPU against its torch restatement (tests/densify_reference.py): the plan's order and counts,
the byte-exact move, densify of a ParameterClass with its optimizer state against `params[keep]` + `append_tensors`,
the 3D split against float64, DensifyStats against index_add_ / index_reduce_, and a short training loop."""
import math

import pytest
import torch

import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import RasterConfig, _native as nv, scenes
from taichi_gaussian_rasterizer_amd.optim import FractionalLaProp, ParameterClass, VisibilityAwareAdam

from densify_reference import (SPLIT_BOUND, log_shrink32, reference_densify, reference_plan, reference_split,
                               same_bits)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# 2049: one row more than a plan workgroup's 2048 rows (256 threads x 8).  698369 = 341 * 2048 + 1: 342 workgroups,
# whose 3 * 342 = 1026 counts are two more than one workgroup of the count scan (gs_full_cumsum_i32: 1024) takes.
PLAN_SIZES = (1, 63, 64, 65, 1000, 2049, 698369)


def random_masks(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, generator=g) < 1 / 3).to(DEV) for _ in range(3)]


def mask_cases(n):
    """name -> (prune, split, clone); None entries reach the library as NULL"""
    off, on = torch.zeros(n, dtype=torch.bool, device=DEV), torch.ones(n, dtype=torch.bool, device=DEV)
    one = off.clone()
    one[n // 2] = True
    p, s, c = random_masks(n, seed=n)
    return {"none": (off, off, off), "all_prune": (on, off, off), "all_split": (off, on, off),
            "all_clone": (off, off, on), "all_set": (on, on, on), "one_prune": (one, off, off),
            "one_split": (off, one, off), "one_clone": (off, off, one), "thirds": (p, s, c),
            "null_prune": (None, s, c), "null_split": (p, None, c), "null_clone": (p, s, None),
            "only_split": (None, s, None), "only_clone": (None, None, c)}


@pytest.mark.parametrize("children", (1, 2, 3))
@pytest.mark.parametrize("n", PLAN_SIZES)
def test_plan_matches_nonzero_order(n, children):
    for name, (prune, split, clone) in mask_cases(n).items():
        want, counts = reference_plan(n, prune, split, clone, children, device=DEV)
        plan = gs.plan_densify(prune, split, clone, children=children)
        got = [plan.kept, plan.clones, plan.split_parents, plan.rows]
        assert got == counts, (name, got, counts)
        assert plan.children == children and plan.num_source == n
        assert plan.src_of.dtype == torch.int32 and plan.src_of.shape == (counts[3],)
        assert torch.equal(plan.src_of.long(), want), name
        if name == "all_prune" or name == "all_set":
            assert plan.rows == 0
    # the kept rows are the boolean index's
    prune, split, clone = mask_cases(n)["thirds"]
    plan = gs.plan_densify(prune, split, clone, children=children)
    assert torch.equal(plan.src_of[:plan.kept].long(), (~(prune | split)).nonzero().flatten())


@pytest.mark.parametrize("n", (65, 2049, 698369))
def test_plan_capacity_smaller_than_rows(n):
    """the counts stay right, entries from `capacity` on are not written"""
    prune, split, clone = random_masks(n, seed=7)
    want, counts = reference_plan(n, prune, split, clone, 3, device=DEV)
    lib = nv.lib()
    need = lib.gs_densify_plan_scratch_bytes(n)
    for capacity in (0, 1, counts[0], counts[0] + counts[1] + 1, counts[3] - 1):
        guard = 64
        src_of = torch.full((capacity + guard,), -7, dtype=torch.int32, device=DEV)
        got = torch.full((4,), -1, dtype=torch.int32, device=DEV)
        scratch = nv.scratch(need, DEV)
        nv.check(lib.gs_densify_plan(n, nv.ptr(prune), nv.ptr(split), nv.ptr(clone), 3, capacity, nv.ptr(src_of),
                                     nv.ptr(got), nv.ptr(scratch), need, nv.stream()), "gs_densify_plan")
        assert got.tolist() == counts, capacity
        assert torch.equal(src_of[:capacity].long(), want[:capacity]), capacity
        assert bool((src_of[capacity:] == -7).all()), capacity
    with pytest.raises(ValueError, match="max_rows"):
        gs.plan_densify(prune, split, clone, children=3, max_rows=counts[3] - 1)
    assert gs.plan_densify(prune, split, clone, children=3, max_rows=counts[3]).rows == counts[3]


# ------------------------------------------------------------------------------------------------------------ move
def raw_floats(shape, seed):
    """float32 with every kind of bit pattern: random words (NaN payloads, denormals, infinities), -0.0 planted"""
    g = torch.Generator().manual_seed(seed)
    words = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, dtype=torch.int64).to(torch.int32)
    flat = words.view(-1)
    flat[0::7] = torch.tensor(-0.0).view(torch.int32)             # -0.0
    flat[1::7] = flat[1::7] & 0x007fffff                          # denormals
    flat[2::7] = flat[2::7] | 0x7fc00000                          # NaNs with payloads
    return words.view(torch.float32).to(DEV)


def move_table(n):
    base = raw_floats((n * 4 + 4,), 10)
    wide = raw_floats((n, 5), 11)
    table = {"f4": raw_floats((n,), 1), "f12": raw_floats((n, 3), 2), "f16": raw_floats((n, 4), 3),
             "f36": raw_floats((n, 3, 3), 4), "f192": raw_floats((n, 3, 16), 5),
             "i64": raw_floats((n, 2), 6).view(torch.int64).view(n), "i64x2": raw_floats((n, 4), 7).view(torch.int64),
             "off4": base[1:1 + 4 * n].view(n, 4),      # 16-byte rows whose storage starts 4 bytes off a 16-byte boundary
             "strided": wide[:, :3],                    # not contiguous: the torch path
             "flag": raw_floats((n,), 8).view(torch.int32) > 0,   # bool: 1-byte rows, the torch path
             "half": raw_floats((n, 3), 9).view(torch.int16)[:, :3].contiguous()}  # 6-byte rows, the torch path
    assert table["off4"].data_ptr() % 16 == 4 and table["off4"].is_contiguous()
    assert n == 1 or not table["strided"].is_contiguous()  # a single row is contiguous whatever its strides
    return table


@pytest.mark.parametrize("n", (1, 1000, 20011))
def test_move_rows_is_a_byte_exact_gather(n):
    table = move_table(n)
    prune, split, clone = random_masks(n, seed=3)
    plan = gs.plan_densify(prune, split, clone, children=2)
    assert plan.rows > 0 or n == 1
    index = plan.src_of.long()
    moved = gs.move_rows(table, plan)
    assert list(moved) == list(table)
    for name, t in table.items():
        assert same_bits(moved[name], t[index]), name
        assert moved[name].is_contiguous()
    # zeros from copy_rows on
    for copy_rows in (0, plan.kept, plan.rows):
        moved = gs.move_rows(table, plan, copy_rows=copy_rows)
        for name, t in table.items():
            want = t[index]
            want[copy_rows:] = 0
            assert same_bits(moved[name], want), (name, copy_rows)
    # records go in as they are
    g3 = gs.Gaussians3D(position=table["f12"], log_scaling=raw_floats((n, 3), 20), rotation=table["f16"],
                        alpha_logit=raw_floats((n, 1), 21), feature=table["f192"])
    moved = gs.move_rows(g3, plan)
    assert same_bits(moved["feature"], table["f192"][index]) and same_bits(moved["alpha_logit"], g3.alpha_logit[index])


def test_move_rows_more_columns_than_one_launch_takes():
    n = 777
    table = {f"c{k}": raw_floats((n, 1 + k % 5), 100 + k) for k in range(nv.GS_MOVE_COLUMNS_MAX + 1)}
    prune, split, clone = random_masks(n, seed=4)
    plan = gs.plan_densify(prune, split, clone, children=3)
    calls = []
    lib = nv.lib()
    inner = lib.gs_table_move_rows
    try:
        lib.gs_table_move_rows = lambda *a: calls.append(a[2]) or inner(*a)
        moved = gs.move_rows(table, plan)
    finally:
        lib.gs_table_move_rows = inner
    assert calls == [32, 1]
    for name, t in table.items():
        assert same_bits(moved[name], t[plan.src_of.long()]), name


# --------------------------------------------------------------------------------------------------------- densify
GROUPS = dict(position=dict(lr=1e-3, type="vector"), log_scaling=dict(lr=1e-3, type="vector"),
              rotation=dict(lr=1e-3, type="vector"), alpha_logit=dict(lr=1e-2, type="scalar"),
              feature=dict(lr=1e-3, type="scalar"))


def sh_scene(n, seed, image_size=(192, 160)):
    """a small 3D scene with SH degree 1 features (n, 3, 4)"""
    torch.manual_seed(seed)
    cam = scenes.random_camera(image_size=image_size)
    g = scenes.random_3d_gaussians(n, cam, scale_factor=1.5)
    g = g.replace(feature=torch.cat([torch.rand(n, 3, 1) * 2, 0.1 * torch.randn(n, 3, 3)], dim=2))
    return g.to(DEV), cam.to(device=DEV)


def render(params, cam, cfg, retain=False):
    g = gs.Gaussians3D(**{name: params.tensors[name] for name in GROUPS}, batch_size=params.batch_size)
    r = gs.render_gaussians(g, cam, cfg, use_sh=True)
    if retain:
        r.gaussians2d.retain_grad()
    return r


def train_steps(params, cam, target, steps, fractional, cfg=RasterConfig(compute_visibility=True)):
    loss = None
    for _ in range(steps):
        params.zero_grad()
        r = render(params, cam, cfg)
        loss = (r.image - target).abs().mean()
        loss.backward()
        if fractional:
            params.step(indexes=r.points_in_view, weight=r.point_visibility.clamp(0, 1))
        else:
            params.step(indexes=r.points_in_view, visibility=r.point_visibility)
    return float(loss)


@pytest.fixture(scope="module", params=["VisibilityAwareAdam", "FractionalLaProp"])
def trained(request):
    """a ParameterClass over 3000 rows after three real steps, its camera, three masks that overlap, the noise"""
    n = 3000
    g, cam = sh_scene(n, seed=11)
    optimizer = VisibilityAwareAdam if request.param == "VisibilityAwareAdam" else FractionalLaProp
    params = ParameterClass(dict(g.items()), GROUPS, optimizer=optimizer)
    target = torch.rand(cam.image_size[1], cam.image_size[0], 3, generator=torch.Generator().manual_seed(5)).to(DEV)
    train_steps(params, cam, target, 3, fractional=optimizer is FractionalLaProp)
    assert all(len(table) >= 2 for table in params.tensor_state.values()) and len(params.tensor_state) == 5
    gen = torch.Generator().manual_seed(6)
    prune, split, clone = ((torch.rand(n, generator=gen) < 0.2).to(DEV) for _ in range(3))
    parents = int((split & ~prune).sum())
    noise = torch.randn(2 * parents, 3, generator=gen).to(DEV)
    return dict(params=params, cam=cam, masks=(prune, split, clone), noise=noise, fractional=optimizer is FractionalLaProp)


def assert_same_parameter_class(ours, ref):
    assert list(ours.tensors) == list(ref.tensors)
    for name in ref.tensors:
        assert same_bits(ours.tensors[name], ref.tensors[name]), name
        assert ours.tensors[name].requires_grad and ours.tensors[name].is_leaf
    ours_state, ref_state = ours.tensor_state, ref.tensor_state
    assert sorted(ours_state) == sorted(ref_state)
    for name, table in ref_state.items():
        assert sorted(ours_state[name]) == sorted(table), name
        for key, t in table.items():
            assert same_bits(ours_state[name][key], t), (name, key)
    assert ours.parameter_groups == ref.parameter_groups
    other, ref_other = ours.other_state, ref.other_state
    assert sorted(other) == sorted(ref_other)
    for name in ref_other:
        assert sorted(other[name]) == sorted(ref_other[name])
        for key, value in ref_other[name].items():
            assert torch.equal(other[name][key], value) if torch.is_tensor(value) else other[name][key] == value


@pytest.mark.parametrize("state", ("zero", "parent"))
def test_densify_equals_the_parameter_class_composition(trained, state):
    params, cam, noise = trained["params"], trained["cam"], trained["noise"]
    prune, split, clone = trained["masks"]
    n = int(params.batch_size[0])
    plan = gs.plan_densify(prune, split, clone, children=2)
    assert plan.split_parents > 0 and plan.clones > 0 and plan.kept < n
    ours = gs.densify(params, plan, noise=noise, shrink=1.6, state=state)
    assert int(ours.batch_size[0]) == plan.rows
    # the source is untouched
    assert int(params.batch_size[0]) == n

    # the children's position against float64, everything else bit for bit
    ref, child64, scale = reference_densify(params, prune, split, clone, 2, noise, 1.6, state)
    first = plan.first_child
    child = ours.tensors["position"].detach()[first:]
    err = (child.double() - child64).abs()
    print(f"split position: max |err| / (|p_i| + ||exp(ls) noise||) = {float((err / scale).max()):.3e} "
          f"(bound {SPLIT_BOUND:.3e})")
    assert bool((err <= SPLIT_BOUND * scale).all())
    ref, _, _ = reference_densify(params, prune, split, clone, 2, noise, 1.6, state, child_position=child)
    assert_same_parameter_class(ours, ref)
    new_rows = plan.rows - plan.kept
    for name, table in ours.tensor_state.items():
        for key, t in table.items():
            fresh = t[plan.kept:]
            assert fresh.shape[0] == new_rows
            if state == "zero":
                assert not bool(fresh.any()), (name, key)

    # one further identical step on both
    gen = torch.Generator().manual_seed(9)
    grads = {name: torch.randn(t.shape, generator=gen).to(DEV) for name, t in ref.tensors.items()}
    rows = torch.arange(0, plan.rows, 3, device=DEV)
    weight = torch.rand(rows.shape[0], generator=gen).to(DEV) * 0.9 + 0.05
    for p in (ours, ref):
        for name, grad in grads.items():
            p.tensors[name].grad = grad.clone()
        p.step(indexes=rows, **{"weight" if trained["fractional"] else "visibility": weight})
    assert_same_parameter_class(ours, ref)

    image = render(ours, cam, RasterConfig()).image
    assert image.shape[2] == 3 and bool(torch.isfinite(image).all())


def test_densify_without_changes_and_to_nothing(trained):
    params = trained["params"]
    n = int(params.batch_size[0])
    off, on = torch.zeros(n, dtype=torch.bool, device=DEV), torch.ones(n, dtype=torch.bool, device=DEV)
    same = gs.densify(params, gs.plan_densify(prune=off))
    assert_same_parameter_class(same, params)
    empty = gs.densify(params, gs.plan_densify(prune=on))
    assert int(empty.batch_size[0]) == 0 and empty.tensors["feature"].shape == (0, 3, 4)
    for table in empty.tensor_state.values():
        assert all(t.shape[0] == 0 for t in table.values())


# ----------------------------------------------------------------------------------------------------------- split
@pytest.mark.parametrize("children", (1, 3))
def test_split_gaussians3d(children):
    n = 777
    g, _ = sh_scene(n, seed=21)
    gen = torch.Generator().manual_seed(22)
    # unnormalised quaternions: the kernel normalises
    g = g.replace(rotation=g.rotation * (0.05 + 20 * torch.rand(n, 1, generator=gen)).to(DEV))
    noise = torch.randn(n, children, 3, generator=gen).to(DEV)
    out = gs.split_gaussians3d(g, noise, shrink=1.6)
    assert len(out) == n * children
    parent_of = torch.arange(n, device=DEV).repeat_interleave(children)
    child64, scale, child_ls = reference_split(g.position, g.log_scaling, g.rotation, parent_of,
                                               noise.view(-1, 3), 1.6)
    assert same_bits(out.log_scaling, child_ls)
    assert same_bits(out.log_scaling, g.log_scaling[parent_of] - torch.tensor(log_shrink32(1.6), device=DEV))
    err = (out.position.double() - child64).abs()
    print(f"split_gaussians3d children={children}: max |err| / scale = {float((err / scale).max()):.3e} "
          f"(bound {SPLIT_BOUND:.3e})")
    assert bool((err <= SPLIT_BOUND * scale).all())
    assert bool(((out.position - g.position[parent_of]).abs().amax(1) > 0).all())  # the children did move
    for name in ("rotation", "alpha_logit", "feature"):
        assert same_bits(getattr(out, name), getattr(g, name)[parent_of]), name
    # no noise: the parent's position, bit for bit
    still = gs.split_gaussians3d(g, torch.zeros_like(noise))
    assert same_bits(still.position, g.position[parent_of])
    assert same_bits(still.log_scaling, child_ls)


# ----------------------------------------------------------------------------------------------------------- stats
@pytest.fixture(scope="module")
def three_views():
    """three views of one scene with visibility, heuristics and the splats' gradients"""
    n = 2000
    g, cam = sh_scene(n, seed=31, image_size=(160, 128))
    # the last 300 rows mirrored through the camera centre: behind every view's camera, listed by none
    behind = g.position.clone()
    behind[-300:] = 2 * cam.camera_position.to(DEV) - behind[-300:]
    g = g.replace(position=behind).requires_grad_(True)
    cfg = RasterConfig(compute_visibility=True, compute_point_heuristic=True)
    views = []
    for k in range(3):
        move = torch.eye(4)
        move[0, 3] = 0.05 * (k - 1)
        r = gs.render_gaussians(g, cam.transformed(move.to(DEV)), cfg, use_sh=True)
        r.gaussians2d.retain_grad()
        target = torch.rand(r.image.shape, generator=torch.Generator().manual_seed(40 + k)).to(DEV)
        (r.image - target).square().mean().backward()
        views.append(r)
    return n, views


def test_stats_match_index_add(three_views):
    n, views = three_views
    stats = gs.DensifyStats(n, DEV)
    assert stats.update(views[0]) is stats
    stats.update(views[1:])
    want = torch.zeros(n, 6, device=DEV)
    grad64 = torch.zeros(n, dtype=torch.float64, device=DEV)
    listed = torch.zeros(n, device=DEV)
    for r in views:
        rows = r.points_in_view
        assert r.gaussians2d.grad is not None and r.gaussians2d.grad.shape == r.gaussians2d.shape
        want[:, 0].index_add_(0, rows, (r.point_visibility > 0).float())
        want[:, 2].index_add_(0, rows, r.point_heuristic[:, 0])
        want[:, 3].index_add_(0, rows, r.point_heuristic[:, 1])
        want[:, 4].index_add_(0, rows, r.point_visibility)
        want[:, 5].index_reduce_(0, rows, r.gaussians2d.detach()[:, 4:6].amax(1), "amax")
        grad64.index_add_(0, rows, r.gaussians2d.grad[:, :2].double().square().sum(1).sqrt())
        listed.index_add_(0, rows, torch.ones_like(r.point_visibility))
    for col, name in ((0, "seen"), (2, "prune_cost"), (3, "split_score"), (4, "visibility"), (5, "max_radius")):
        assert same_bits(getattr(stats, name), want[:, col]), name
    # per update: the squares and their sum, the square root, the add to the running sum: 3 roundings of 2^-24 relative
    # to a value no larger than the final sum
    bound = 3 * 2.0 ** -24 * listed.double() * grad64
    err = (stats.viewspace_grad.double() - grad64).abs()
    print(f"viewspace_grad: max err / bound = {float((err / bound.clamp(min=1e-300)).max()):.3f}, "
          f"rows with a gradient {int((grad64 > 0).sum())}")
    assert bool((err <= bound).all())
    assert int((grad64 > 0).sum()) > n // 10 and float(stats.split_score.abs().sum()) > 0
    unlisted = listed == 0
    assert int(unlisted.sum()) >= 300 and not bool(stats.stats[unlisted].any())
    seen = stats.seen.clamp(min=1)
    assert torch.equal(stats.mean_viewspace_grad, stats.viewspace_grad / seen)
    assert not bool(stats.reset().stats.any())


def test_stats_null_inputs_leave_their_columns(three_views):
    n, views = three_views
    r = views[0]
    rows, v = r.points_in_view, r.points_in_view.shape[0]
    start = torch.arange(6.0, device=DEV).repeat(n, 1) + 0.5

    def after(**inputs):
        stats = gs.DensifyStats(n, DEV)
        stats.stats.copy_(start)
        return stats.update_rows(rows, **inputs).stats

    got = after()  # nothing but the list: every listed row counts as seen
    assert torch.equal(got[:, 1:], start[:, 1:]) and torch.equal(got[rows, 0], start[rows, 0] + 1)
    got = after(visibility=r.point_visibility)
    assert torch.equal(got[:, [1, 2, 3, 5]], start[:, [1, 2, 3, 5]])
    assert torch.equal(got[rows, 0], start[rows, 0] + (r.point_visibility > 0).float())
    assert torch.equal(got[rows, 4], start[rows, 4] + r.point_visibility)
    got = after(heuristic=r.point_heuristic)
    assert torch.equal(got[:, [1, 4, 5]], start[:, [1, 4, 5]])
    assert torch.equal(got[rows, 2], start[rows, 2] + r.point_heuristic[:, 0])
    assert torch.equal(got[rows, 3], start[rows, 3] + r.point_heuristic[:, 1])
    got = after(gaussians2d=r.gaussians2d)
    assert torch.equal(got[:, 1:5], start[:, 1:5])
    assert torch.equal(got[rows, 5], torch.maximum(start[rows, 5], r.gaussians2d.detach()[:, 4:6].amax(1)))
    # a (V, 2) gradient and the first two columns of a (V, 7) one are the same input
    a, b = after(grad2d=r.gaussians2d.grad), after(grad2d=r.gaussians2d.grad[:, :2].contiguous())
    assert torch.equal(a, b) and torch.equal(a[:, 2:], start[:, 2:]) and bool((a[rows, 1] >= start[rows, 1]).all())
    # tiny gradients do not vanish in the squares
    tiny = torch.full((v, 2), 3e-30, device=DEV)
    got = gs.DensifyStats(n, DEV).update_rows(rows, grad2d=tiny).viewspace_grad[rows]
    assert torch.allclose(got, torch.full_like(got, 3e-30 * math.sqrt(2)), rtol=1e-6, atol=0)
    other = torch.ones(n, dtype=torch.bool, device=DEV)
    other[rows] = False
    assert torch.equal(after(visibility=r.point_visibility, heuristic=r.point_heuristic, gaussians2d=r.gaussians2d,
                             grad2d=r.gaussians2d.grad)[other], start[other])


# ------------------------------------------------------------------------------------------------------ a short loop
def test_training_loop_with_densification():
    n = 2000
    g, cam = sh_scene(n, seed=51, image_size=(160, 128))
    params = ParameterClass(dict(g.items()), GROUPS, optimizer=VisibilityAwareAdam)
    target = torch.rand(cam.image_size[1], cam.image_size[0], 3, generator=torch.Generator().manual_seed(52)).to(DEV)
    cfg = RasterConfig(compute_visibility=True, compute_point_heuristic=True)
    stats = gs.DensifyStats(n, DEV)
    sizes = [n]
    for it in range(1, 31):
        before = params.tensors["feature"].detach().clone()
        params.zero_grad()
        r = render(params, cam, cfg, retain=True)
        loss = (r.image - target).abs().mean()
        loss.backward()
        params.step(indexes=r.points_in_view, visibility=r.point_visibility)
        assert math.isfinite(float(loss))
        assert not torch.equal(params.tensors["feature"].detach(), before)  # the optimizer keeps stepping
        stats.update(r)
        if it % 10 == 0:
            count = stats.num_points
            signal = stats.mean_viewspace_grad
            prune = (stats.seen == 0) | (stats.visibility < stats.visibility.quantile(0.05))
            grow = signal >= signal.quantile(0.85)
            large = stats.max_radius > stats.max_radius.median()
            plan = gs.plan_densify(prune, grow & large, grow & ~large, children=2)
            assert plan.split_parents > 0 and plan.clones > 0 and plan.kept < count
            params = gs.densify(params, plan)
            assert int(params.batch_size[0]) == plan.rows
            assert plan.rows == plan.kept + plan.clones + 2 * plan.split_parents
            sizes.append(plan.rows)
            stats = gs.DensifyStats(plan.rows, DEV)
    assert len(sizes) == 4 and len(set(sizes)) == 4
