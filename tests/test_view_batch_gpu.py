"""One optimizer step after several backward passes: the ascending runs of a summed gradient's index list
(gs_rows_find_runs), the rows of a step summed run by run (gs_rows_sum_runs), the union of the views' visible sets
(gs_rows_union), and the optimizers and helpers on top of them (optim.gather_sparse_grad, union_rows, visible_union,
fractional.MERGE_RUNS).  Expected values come from numpy / torch on the CPU: the sequential float32 accumulation
`acc = zeros(N, D); for each run in order: acc[rows of the run] += values of the run`, exact per run because a run's rows
are distinct."""
import ctypes

import numpy as np
import pytest
import torch

import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import RasterConfig, _native as nv, optim, scenes
from taichi_gaussian_rasterizer_amd.optim import fractional, rows as row_lists

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
N = 5000
MAX_RUNS = row_lists.MAX_RUNS
BLOCK = 256  # the workgroup size of rows.hip's kernels


# ------------------------------------------------------------------------------------------------- restatements
def np_runs(rows, max_runs=MAX_RUNS):
    """(run_count, run_starts (max_runs + 1)) as include/gsplat_hip.h states them"""
    rows = np.asarray(rows, dtype=np.int64)
    count = rows.shape[0]
    starts = [0] + [i for i in range(1, count) if rows[i] <= rows[i - 1]] if count else []
    expect = np.full(max_runs + 1, count, dtype=np.int64)
    keep = min(len(starts), max_runs + 1)
    expect[:keep] = starts[:keep]
    return len(starts), expect


def split_runs(rows):
    count, starts = np_runs(rows, max_runs=len(rows) + 1)
    bounds = list(starts[:count]) + [len(rows)]
    return [(int(bounds[k]), int(bounds[k + 1])) for k in range(count)]


def sequential_sum(n, rows, values):
    """the (n, D) float32 accumulation of `values` (R, D) at `rows` (R), run by run in order; rows outside [0, n) are
    skipped"""
    acc = torch.zeros((n, values.shape[1]), dtype=torch.float32)
    for lo, hi in split_runs(rows.numpy()):
        idx, val = rows[lo:hi], values[lo:hi]
        inside = (idx >= 0) & (idx < n)
        acc[idx[inside]] += val[inside]  # distinct rows: no repeated index in one statement
    return acc


def device_runs(rows, max_runs=MAX_RUNS):
    lib = nv.lib()
    dev = torch.as_tensor(rows, dtype=torch.int64).to(DEV)
    starts = torch.full((max_runs + 1,), -7, dtype=torch.int64, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    nv.check(lib.gs_rows_find_runs(dev.shape[0], nv.ptr(dev), max_runs, nv.ptr(starts), nv.ptr(count), nv.stream()),
             "gs_rows_find_runs")
    return int(count.item()), starts.cpu().numpy()


def ascending(gen, size, low=0, high=N):
    return (torch.randperm(high - low, generator=gen)[:size] + low).sort().values


# ------------------------------------------------------------------------------------------------- 1. runs
def _run_lists():
    gen = torch.Generator().manual_seed(11)
    lists = {"one": [17], "ascending1000": list(range(3, 3003, 3)), "equal_neighbours": [1, 4, 4, 7],
             "all_equal": [5] * 70}
    for lengths in ((1, 64, 65), (63, 1, 1500)):
        lists[f"lengths{lengths}"] = torch.cat([ascending(gen, k) for k in lengths]).tolist()
    # descents at, just before and just behind every multiple of 64 (and so of the workgroup size), in a list three
    # workgroups long plus one
    count = 3 * BLOCK + 1
    for delta in (-1, 0, 1):
        at = sorted({64 * m + delta for m in range(1, count // 64 + 1)} & set(range(1, count)))
        bounds = [0] + at + [count]
        lists[f"descents{delta:+d}"] = [i for lo, hi in zip(bounds[:-1], bounds[1:]) for i in range(hi - lo)]
    return lists


RUN_LISTS = _run_lists()


@pytest.mark.parametrize("name", sorted(RUN_LISTS))
def test_find_runs_matches_restatement(name):
    rows = RUN_LISTS[name]
    for max_runs in (MAX_RUNS, 1, 3):
        count, starts = device_runs(rows, max_runs)
        expect_count, expect = np_runs(rows, max_runs)
        assert count == expect_count, (name, max_runs)
        assert np.array_equal(starts, expect), (name, max_runs, starts, expect)
    if name.startswith("descents"):
        assert np_runs(rows)[0] == (13 if name != "descents+1" else 12) and len(rows) == 3 * BLOCK + 1


def test_find_runs_counts_more_runs_than_it_lists():
    rows = list(range(40, 0, -1))
    count, starts = device_runs(rows, MAX_RUNS)
    assert count == 40 and np.array_equal(starts, np.arange(MAX_RUNS + 1))
    # random order: about half the elements start a run; the count is exact and the listed starts are the first ones
    rows = torch.randperm(3000, generator=torch.Generator().manual_seed(3)).tolist()
    count, starts = device_runs(rows, MAX_RUNS)
    expect_count, expect = np_runs(rows)
    assert count == expect_count > 1000 and np.array_equal(starts, expect)


def test_empty_calls_write_nothing():
    lib = nv.lib()
    starts = torch.full((MAX_RUNS + 1,), -7, dtype=torch.int64, device=DEV)
    count = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    assert lib.gs_rows_find_runs(0, None, MAX_RUNS, nv.ptr(starts), nv.ptr(count), nv.stream()) == 0
    assert lib.gs_rows_union(100, 0, None, nv.ptr(starts), nv.ptr(count), None, 0, nv.stream()) == 0
    assert lib.gs_rows_sum_runs(0, None, 3, None, 10, None, 3, None, nv.ptr(starts), nv.stream()) == 0
    torch.cuda.synchronize()
    assert bool((starts == -7).all()) and bool((count == -7).all())
    empty = torch.empty(0, dtype=torch.int64, device=DEV)
    rows, summed = optim.union_rows([empty, empty], [empty.float(), empty.float()], num_points=10)
    assert rows.shape == (0,) and rows.dtype == torch.int64 and summed.shape == (0,)


# ------------------------------------------------------------------------------------------------- 2. sum over runs
SIZES = (1, 63, 64, 65, 1500)
COMMON = 2500  # a row every run lists


def _make_runs(num_runs, seed):
    """`num_runs` ascending lists of distinct rows of range(N), sizes cycling through SIZES, each holding COMMON: their
    concatenation has exactly that many runs (a run cannot continue into the next list: both hold COMMON)"""
    gen = torch.Generator().manual_seed(seed)
    first = int(torch.randint(len(SIZES), (1,), generator=gen))
    lists = []
    for b in range(num_runs):
        rows = ascending(gen, SIZES[(first + b) % len(SIZES)])
        lists.append(torch.unique(torch.cat([rows, torch.tensor([COMMON])])))
    return lists, gen


def _index_shapes(lists, gen):
    union = torch.unique(torch.cat(lists))
    member = torch.zeros(N, dtype=torch.bool)
    member[union] = True
    outside = torch.nonzero(~member).flatten()
    extra = outside[torch.randperm(outside.shape[0], generator=gen)[:100]]
    more = torch.cat([union, extra]).sort().values
    return {"union": union, "union_plus_unlisted": more,
            "permuted": more[torch.randperm(more.shape[0], generator=gen)]}


@pytest.mark.parametrize("dims", [1, 3, 4, 30, 48])
@pytest.mark.parametrize("num_runs", [1, 2, 3, 16])
def test_sum_runs_equals_sequential_accumulation(num_runs, dims):
    lists, gen = _make_runs(num_runs, 100 * num_runs + dims)
    cat = torch.cat(lists)
    values = torch.randn(cat.shape[0], dims, generator=gen)
    expect = sequential_sum(N, cat, values)
    cat_dev, values_dev = cat.to(DEV), values.to(DEV)
    starts, count = row_lists.find_runs(cat_dev)
    assert int(count.item()) == num_runs
    assert np.array_equal(starts.cpu().numpy(), np_runs(cat.numpy())[1])
    # the same values 4 bytes off a 16-byte boundary: the kernels then take their 4-byte accesses
    shifted = torch.empty(values.numel() + 1, device=DEV)[1:].view(values.shape).copy_(values_dev)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for shape, indexes in _index_shapes(lists, gen).items():
        for run in lists:  # the first and last row of every run, and the row in all of them, are asked for
            assert bool((indexes == run[0]).any()) and bool((indexes == run[-1]).any())
        assert bool((indexes == COMMON).any())
        for vals in (values_dev, shifted):
            got = row_lists.sum_runs(indexes.to(DEV), num_runs, starts, cat_dev, vals)
            assert got.shape == (indexes.shape[0], dims)
            assert torch.equal(got.cpu(), expect[indexes]), (shape, (got.cpu() - expect[indexes]).abs().max())
    indexes = torch.unique(cat)
    assert float(expect[COMMON].abs().sum()) > 0
    none = row_lists.sum_runs(indexes.to(DEV), 0, None, torch.empty(0, dtype=torch.int64, device=DEV),
                              torch.empty(0, dims, device=DEV))
    assert none.shape == (indexes.shape[0], dims) and float(none.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------- 3. union
def _union_lists(num_lists, seed):
    lists, gen = _make_runs(num_lists, seed)
    lists[0] = torch.cat([lists[0], lists[0][:2], torch.tensor([-1, N, COMMON, N + 70, -1])])  # repeats, out of range
    if num_lists > 1:
        half = lists[1].shape[0] // 2
        lists[1] = torch.cat([lists[1][half:], lists[1][:half]])  # a list need not ascend
    return lists, gen


@pytest.mark.parametrize("num_lists", [1, 2, 3, 6])
def test_union_rows_and_summed_values(num_lists):
    lists, gen = _union_lists(num_lists, 40 + num_lists)
    values = [torch.randn(rows.shape[0], generator=gen) for rows in lists]
    cat, vcat = torch.cat(lists), torch.cat(values)
    assert num_lists < np_runs(cat.numpy(), len(cat))[0] <= MAX_RUNS  # the kernels' path, more runs than lists
    inside = cat[(cat >= 0) & (cat < N)]
    assert inside.shape[0] < cat.shape[0]
    rows, summed = optim.union_rows([r.to(DEV) for r in lists], [v.to(DEV) for v in values], num_points=N)
    assert rows.dtype == torch.int64 and torch.equal(rows.cpu(), torch.unique(inside))
    expect = sequential_sum(N, cat, vcat.unsqueeze(1))[:, 0]
    assert torch.equal(summed.cpu(), expect[rows.cpu()])
    only_rows, nothing = optim.union_rows([r.to(DEV) for r in lists], num_points=N)
    assert nothing is None and torch.equal(only_rows, rows)
    # a bitmap that is no multiple of anything: the last row, and a universe that ends inside a word
    small = optim.union_rows([torch.tensor([32, 0, 31, 32, 33], device=DEV)], num_points=33)[0]
    assert small.tolist() == [0, 31, 32]


def test_union_rows_beyond_one_workgroup_of_the_bitmap():
    """a universe of several bitmap workgroups (32768 rows each), rows at their edges"""
    n = 3 * 32768 + 5
    edges = [0, 31, 32, 127, 128, 32767, 32768, 32769, 2 * 32768 - 1, 2 * 32768, 3 * 32768, n - 1]
    gen = torch.Generator().manual_seed(9)
    a = torch.unique(torch.cat([torch.tensor(edges), torch.randint(n, (4000,), generator=gen)]))
    b = torch.unique(torch.randint(n, (3000,), generator=gen))
    va, vb = torch.randn(a.shape[0], generator=gen), torch.randn(b.shape[0], generator=gen)
    rows, summed = optim.union_rows([a.to(DEV), b.to(DEV)], [va.to(DEV), vb.to(DEV)], num_points=n)
    assert torch.equal(rows.cpu(), torch.unique(torch.cat([a, b])))
    expect = sequential_sum(n, torch.cat([a, b]), torch.cat([va, vb]).unsqueeze(1))[:, 0]
    assert torch.equal(summed.cpu(), expect[rows.cpu()])


def test_union_rows_falls_back_beyond_max_runs(monkeypatch):
    """17 lists: more runs than gs_rows_sum_runs takes, so torch.unique and index_add_, whose order of addition is not
    fixed -- the values are multiples of 2^-8 in [-4, 4], which every order sums to the same float"""
    lists, gen = _make_runs(MAX_RUNS + 1, 77)
    lists[-1] = torch.cat([lists[-1], torch.tensor([-1, N])])
    values = [torch.randint(-1024, 1025, (rows.shape[0],), generator=gen) / 256.0 for rows in lists]
    calls = []
    real = row_lists._union_torch
    monkeypatch.setattr(row_lists, "_union_torch", lambda *a: calls.append(1) or real(*a))
    rows, summed = optim.union_rows([r.to(DEV) for r in lists], [v.to(DEV) for v in values], num_points=N)
    assert calls == [1]
    cat, vcat = torch.cat(lists), torch.cat(values)
    assert torch.equal(rows.cpu(), torch.unique(cat[(cat >= 0) & (cat < N)]))
    assert torch.equal(summed.cpu(), sequential_sum(N, cat, vcat.unsqueeze(1))[rows.cpu(), 0])
    # the same lists, one fewer: the kernels' path, the same answer
    calls.clear()
    rows16, summed16 = optim.union_rows([r.to(DEV) for r in lists[:-1]], [v.to(DEV) for v in values[:-1]], num_points=N)
    assert calls == []
    cat, vcat = torch.cat(lists[:-1]), torch.cat(values[:-1])
    assert torch.equal(summed16.cpu(), sequential_sum(N, cat, vcat.unsqueeze(1))[rows16.cpu(), 0])
    # MERGE_RUNS = False: the torch path whatever the number of runs
    monkeypatch.setattr(fractional, "MERGE_RUNS", False)
    rows_off, summed_off = optim.union_rows([r.to(DEV) for r in lists[:-1]], [v.to(DEV) for v in values[:-1]],
                                            num_points=N)
    assert calls == [1] and torch.equal(rows_off, rows16) and torch.equal(summed_off, summed16)


def test_union_rows_type_checks_device_tensors():
    a = torch.tensor([1, 4, 7], device=DEV)
    with pytest.raises(TypeError):
        optim.union_rows([a.to(torch.int32)], num_points=10)
    with pytest.raises(TypeError):
        optim.union_rows([a], [torch.ones(3, dtype=torch.float64, device=DEV)], num_points=10)
    with pytest.raises(AssertionError):
        optim.union_rows([a], [torch.ones(2, device=DEV)], num_points=10)
    with pytest.raises(RuntimeError):
        optim.union_rows([a], [torch.ones(3)], num_points=10)


# ------------------------------------------------------------------------------------------------- 4. optimizers
OPTIMIZERS = {"FractionalAdam": False, "FractionalLaProp": False, "VisibilityAwareAdam": True,
              "VisibilityAwareLaProp": True}


def _twins(name, n, seed):
    from test_optim_gpu import _groups
    params, types = _groups(n, seed)  # position: local_vector; log_scaling, rotation: vector; the rest: scalar
    assert set(types.values()) == {"scalar", "vector", "local_vector"}
    lrs = dict(position=0.01, log_scaling=0.02, rotation=0.005, alpha_logit=0.05, feature=0.03)
    gen = torch.Generator().manual_seed(seed + 1)
    mask_lr = torch.rand(3, 4, generator=gen)
    point_lr = torch.rand(n, generator=gen) + 0.5
    out = []
    for _ in range(2):
        dev_params = {k: torch.nn.Parameter(v.clone().to(DEV)) for k, v in params.items()}
        groups = [dict(params=[dev_params[k]], name=k, type=types[k], lr=lrs[k],
                       mask_lr=mask_lr.to(DEV) if k == "feature" else None,
                       point_lr=point_lr.to(DEV) if k == "position" else None) for k in params]
        out.append((dev_params, getattr(optim, name)(groups, betas=(0.9, 0.999))))
    return out, gen


def _assert_same_bits(a, b, what):
    (pa, oa), (pb, ob) = a, b
    for k in pa:
        assert torch.equal(pa[k], pb[k]), (what, k, (pa[k] - pb[k]).abs().max())
        sa, sb = oa.state[pa[k]], ob.state[pb[k]]
        assert set(sa) == set(sb) and {"v", "m"} <= set(sa), (what, k, set(sa), set(sb))
        for key in sa:
            assert torch.equal(sa[key], sb[key]), (what, k, key)


def _refuse_coalesce(self):
    raise AssertionError("coalesce() was called")


def _steps(name, num_runs, monkeypatch, patch):
    """three steps of twin A from hand-built uncoalesced gradients of `num_runs` runs against twin B from the same
    gradients coalesced beforehand; `patch(monkeypatch)` is applied around twin A's steps only"""
    n = 3000
    (a, b), gen = _twins(name, n, 5)
    start = a[0]["feature"].detach().clone()
    for step in range(3):
        lists, _ = _make_runs(num_runs, 1000 * step + num_runs)
        lists = [rows[rows < n] for rows in lists]
        cat = torch.cat(lists).to(DEV)
        for k, p in a[0].items():
            # multiples of 2^-8 in [-4, 4]: every order of summation gives the same float
            vals = (torch.randint(-1024, 1025, (cat.shape[0], *p.shape[1:]), generator=gen) / 256.0).to(DEV)
            grad = torch.sparse_coo_tensor(cat[None], vals, p.shape)
            assert not grad.is_coalesced()
            p.grad = grad
            b[0][k].grad = grad.coalesce()
        union = torch.unique(torch.cat(lists))
        idx = union[torch.rand(union.shape[0], generator=gen) < 0.8]
        idx = torch.cat([idx, torch.tensor([7, 11])]).unique()  # most listed rows, and some the gradient may not list
        w = torch.rand(idx.shape[0], generator=gen) * 0.9 + 0.05
        q = torch.linalg.qr(torch.randn(idx.shape[0], 3, 3, generator=gen)).Q * \
            (0.5 + torch.rand(idx.shape[0], 1, 1, generator=gen))
        b[1].step(idx.to(DEV), w.to(DEV), basis=q.to(DEV))
        with monkeypatch.context() as m:
            patch(m)
            a[1].step(idx.to(DEV), w.to(DEV), basis=q.to(DEV))
        assert all(p.grad.is_sparse and not p.grad.is_coalesced() for p in a[0].values())
    _assert_same_bits(a, b, f"{name}/{num_runs} runs")
    assert not torch.equal(a[0]["feature"].detach(), start)


@pytest.mark.parametrize("name", sorted(OPTIMIZERS))
def test_optimizers_step_from_runs_without_coalesce(name, monkeypatch):
    _steps(name, 3, monkeypatch, lambda m: m.setattr(torch.Tensor, "coalesce", _refuse_coalesce))


def _spy(calls):
    real = torch.Tensor.coalesce

    def coalesce(self):
        calls.append(1)
        return real(self)
    return coalesce


@pytest.mark.parametrize("name", sorted(OPTIMIZERS))
def test_optimizers_coalesce_beyond_max_runs(name, monkeypatch):
    calls = []
    _steps(name, MAX_RUNS + 1, monkeypatch, lambda m: m.setattr(torch.Tensor, "coalesce", _spy(calls)))
    assert len(calls) >= 3 * 5  # every group of every step


@pytest.mark.parametrize("name", ["FractionalLaProp", "VisibilityAwareAdam"])
def test_merge_runs_switch_off_is_the_coalesce_path(name, monkeypatch):
    calls = []
    monkeypatch.setattr(fractional, "MERGE_RUNS", False)
    _steps(name, 3, monkeypatch, lambda m: m.setattr(torch.Tensor, "coalesce", _spy(calls)))
    assert len(calls) >= 3 * 5


def test_gather_sparse_grad_takes_the_three_paths(monkeypatch):
    lists, gen = _make_runs(3, 21)
    cat = torch.cat(lists)
    values = torch.randint(-1024, 1025, (cat.shape[0], 3, 4), generator=gen) / 256.0
    grad = torch.sparse_coo_tensor(cat[None].to(DEV), values.to(DEV), (N, 3, 4))
    expect = sequential_sum(N, cat, values.reshape(-1, 12))
    indexes = torch.cat([torch.unique(cat)[::2], torch.tensor([0, N - 1])]).unique()
    coalesced = grad.coalesce()
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "coalesce", _refuse_coalesce)
        for g in (grad, coalesced):  # runs; an ascending list read in place
            got = optim.gather_sparse_grad(g, indexes.to(DEV))
            assert got.shape == (indexes.shape[0], 12) and torch.equal(got.cpu(), expect[indexes])
        whole = optim.gather_sparse_grad(coalesced, coalesced._indices()[0])
        assert torch.equal(whole.cpu(), expect[coalesced._indices()[0].cpu()])
    calls = []
    many = torch.sparse_coo_tensor(cat.flip(0)[None].to(DEV), values.flip(0).to(DEV), (N, 3, 4))  # mostly descending
    monkeypatch.setattr(torch.Tensor, "coalesce", _spy(calls))
    got = optim.gather_sparse_grad(many, indexes.to(DEV))
    assert calls == [1] and torch.equal(got.cpu(), expect[indexes])
    with pytest.raises(TypeError):
        optim.gather_sparse_grad(torch.zeros(4, 3, device=DEV), indexes.to(DEV))


def test_bench_view_batch_runs_at_a_small_size():
    from taichi_gaussian_rasterizer_amd.benchmarks import bench_view_batch as bench
    args = bench.parse_args(["--n", "20000", "--iters", "2", "--image_size", "256,192", "--degree", "1"])
    g, cam = bench.make_scene(args, 1)
    switch = fractional.MERGE_RUNS
    try:
        out = bench.bench_batch(args, g, cam, 3, warmup=1, rounds=1)
    finally:
        fractional.MERGE_RUNS = switch
    assert out["N"] == 40000 and len(out["V"]) == 3 and max(out["V"]) <= out["union"] <= sum(out["V"])
    assert len(set(out["V"])) > 1, "the cameras see the same rows"
    for mode in ("coalesce", "merge_runs"):
        for part in ("iteration", "step"):
            assert np.isfinite(out[mode][part]["ms"]) and out[mode][part]["ms"] > 0
        assert out[mode]["step"]["ms"] < out[mode]["iteration"]["ms"]


# ------------------------------------------------------------------------------------------------- 5. end to end
def test_three_views_into_one_step(monkeypatch):
    from taichi_gaussian_rasterizer_amd.fused import is_frame_sparse_grad
    n, size, B = 3000, (96, 64), 3
    g, cam = scenes.benchmark_scene(n, size, sh_degree=1)
    cams = [cam]
    for dx in (0.02, -0.03):
        move = torch.eye(4)
        move[0, 3] = dx
        cams.append(cam.transformed(move))
    params = {k: torch.nn.Parameter(v.clone().to(DEV)) for k, v in g.items()}
    kinds = (("position", 1e-3, "vector"), ("log_scaling", 1e-2, "vector"), ("rotation", 1e-2, "vector"),
             ("alpha_logit", 1e-1, "scalar"), ("feature", 1e-2, "scalar"))
    opt = optim.VisibilityAwareAdam([dict(params=[params[k]], name=k, lr=lr, type=t) for k, lr, t in kinds])
    per_view = {k: [] for k in params}  # each backward's own gradient, dense float64, as the leaf receives it
    for k, p in params.items():
        p.register_hook(lambda grad, k=k: per_view[k].append(grad.to_dense().double().cpu()) and None)
    cfg = RasterConfig(compute_visibility=True)
    gen = torch.Generator().manual_seed(4)
    opt.zero_grad()
    rs = [gs.render_gaussians(type(g)(**params, batch_size=(n,)), c.to(device=DEV), cfg, use_sh=True, sparse_grad=True)
          for c in cams]
    for r in rs:
        target = torch.rand(size[1], size[0], 3, generator=gen).to(DEV)
        torch.nn.functional.l1_loss(r.image, target).backward()
    seen = [r.points_in_view.cpu() for r in rs]
    assert all(0 < s.shape[0] < n for s in seen) and not torch.equal(seen[0], seen[1]) \
        and not torch.equal(seen[0], seen[2])
    for k, p in params.items():
        assert p.grad.is_sparse and not is_frame_sparse_grad(p.grad), k
        assert len(per_view[k]) == B
    indexes, visibility = optim.visible_union(rs)
    assert torch.equal(indexes.cpu(), torch.unique(torch.cat(seen)))
    same = optim.visible_union(rs, num_points=n)
    assert torch.equal(same[0], indexes) and torch.equal(same[1], visibility)
    acc = torch.zeros(n)
    for r, s in zip(rs, seen):
        acc[s] += r.point_visibility.detach().cpu()
    assert torch.equal(visibility.cpu(), acc[indexes.cpu()])
    at = indexes.cpu()
    for k, p in params.items():
        got = optim.gather_sparse_grad(p.grad, indexes).cpu().double()
        views = [d.reshape(n, -1)[at] for d in per_view[k]]
        total, magnitude = sum(views), sum(v.abs() for v in views)
        # recursive summation of B float32 terms: |error| <= (B - 1) u sum|g_b| to first order, u = 2^-24
        bound = B * 2.0 ** -24 * magnitude
        assert float(magnitude.max()) > 0, k
        assert bool(((got - total).abs() <= bound).all()), (k, float(((got - total).abs() - bound).max()))
    before = {k: p.detach().clone() for k, p in params.items()}
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "coalesce", _refuse_coalesce)
        opt.step(*optim.visible_union(rs))
    torch.cuda.synchronize()
    for k, p in params.items():
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), before[k]), k
        untouched = torch.ones(n, dtype=torch.bool)
        untouched[at] = False
        assert torch.equal(p.detach().cpu()[untouched], before[k].cpu()[untouched]), k
