"""The MCMC strategy on the GPU against its numpy restatement (tests/mcmc_reference.py): the draw bit for bit, the
correction against float64, the perturbation within its derived bound, relocate and grow of a trained ParameterClass
against the composition on plain arrays, and a short training loop."""
import math

import numpy as np
import pytest
import torch

import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import RasterConfig, losses, scenes
from taichi_gaussian_rasterizer_amd.optim import FractionalLaProp, ParameterClass, VisibilityAwareAdam

from densify_reference import same_bits
from mcmc_reference import (VALUE_TOL, perturb_bound, reference_grow, reference_perturb, reference_relocate,
                            reference_sample, reference_values)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# 2049: one row more than a scan workgroup's 2048.  698369 = 341 * 2048 + 1: 342 workgroup sums.  2097153 =
# 1024 * 2048 + 1: 1025 sums, one more than the sums pass takes in one step of 1024 (it has no limit beyond that:
# further steps repeat the second one).
SAMPLE_SIZES = (1, 64, 65, 2049, 698369, 2097153)
BELOW = float(np.nextafter(np.float32(2.0 ** -24), np.float32(0)))
SPECIALS = (0.0, 1.0, 2.5, -1.0, math.nan, 1e-42, 2.0 ** -24, BELOW, -0.0, math.inf)


def sample_weights(n, seed):
    """random weights in [0, 1) with the special values planted mid-table and runs of zeros at both ends"""
    w = torch.rand(n, generator=torch.Generator().manual_seed(seed))
    if n >= 64:
        run = n // 16
        w[:run] = 0
        w[n - run:] = 0
        w[n // 2:n // 2 + len(SPECIALS)] = torch.tensor(SPECIALS)
        w[n // 3] = 2.0 ** -24  # a row of weight one unit among ordinary rows
    return w


def random_words(m, seed):
    r = torch.randint(0, 2 ** 32, (m,), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)
    r[0] = 0
    r[-1] = 2 ** 32 - 1
    if m > 2:
        r[m // 2] = 2 ** 32 - 1
        r[m // 2 - 1] = 0
    return r


def check_sample(w, r, exclude=None, select=None):
    want_rows, want_copies = reference_sample(w.numpy(), r.numpy(), None if exclude is None else exclude.numpy(),
                                              None if select is None else select.numpy())
    rows, copies = gs.sample_rows(w.to(DEV), r.shape[0], random=r.to(DEV),
                                  exclude=None if exclude is None else exclude.to(DEV),
                                  select=None if select is None else select.to(DEV))
    assert rows.dtype == torch.int32 and copies.dtype == torch.int32
    assert rows.shape == (r.shape[0],) and copies.shape == (w.shape[0],)
    assert np.array_equal(rows.cpu().numpy(), want_rows)
    assert np.array_equal(copies.cpu().numpy(), want_copies)
    return want_rows, want_copies


@pytest.mark.parametrize("n", SAMPLE_SIZES)
def test_sampling_is_bit_exact(n):
    w = sample_weights(n, seed=n)
    g = torch.Generator().manual_seed(n + 1)
    m = 4097  # draws are independent of the table: more than one workgroup of them, and not a multiple of one
    rows, copies = check_sample(w, random_words(m, n + 2))
    assert int(copies.sum()) == m
    exclude = torch.rand(n, generator=g) < 0.3
    check_sample(w, random_words(m, n + 3), exclude=exclude)
    # one draw per row, only where selected; as relocate calls it, the selected rows are excluded
    select = torch.rand(n, generator=g) < 0.1
    select[0] = select[-1] = True
    rows, copies = check_sample(w, random_words(n, n + 4), exclude=select, select=select)
    unselected = ~select.numpy()
    assert np.array_equal(rows[unselected], np.arange(n)[unselected])
    assert not copies[select.numpy()].any()
    check_sample(w, random_words(n, n + 5), exclude=exclude, select=select)  # selected rows may be drawn here
    # int32 bit patterns are the same words
    r = random_words(m, n + 6)
    a = gs.sample_rows(w.to(DEV), m, random=r.to(DEV))
    b = gs.sample_rows(w.to(DEV), m, random=r.to(torch.int32).to(DEV))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("n", (1, 65, 2049))
def test_sampling_without_a_drawable_row_is_a_no_op(n):
    for w in (torch.zeros(n), torch.full((n,), BELOW), torch.full((n,), math.nan), -torch.rand(n)):
        rows, copies = check_sample(w, random_words(n, 3))
        assert np.array_equal(rows, np.arange(n)) and not copies.any()
        select = torch.ones(n, dtype=torch.bool)
        check_sample(w, random_words(n, 4), select=select)
    w = sample_weights(n, 5)
    everything = torch.ones(n, dtype=torch.bool)
    rows, copies = check_sample(w, random_words(n, 6), exclude=everything, select=everything)
    assert np.array_equal(rows, np.arange(n)) and not copies.any()
    rows, copies = gs.sample_rows(w.to(DEV), 0)
    assert rows.shape == (0,) and copies.shape == (n,) and not bool(copies.any())


# ------------------------------------------------------------------------------------------------------ correction
OPACITIES = (1e-6, 0.005, 0.3, 0.95, 0.999999, 1.0)
COPIES = (1, 2, 9, 50, 51, 500)


def test_relocation_values_against_float64():
    o = torch.tensor([o for o in OPACITIES for _ in COPIES], dtype=torch.float32)
    copies = torch.tensor([c for _ in OPACITIES for c in COPIES], dtype=torch.int32)
    assert float(o[-1]) == 1.0
    ls = (torch.rand(o.shape[0], 3, generator=torch.Generator().manual_seed(1)) * 9 - 7)
    want_alpha, want_ls = reference_values(o.numpy(), ls.numpy(), copies.numpy())
    alpha, new_ls = gs.relocation_values(o.to(DEV), ls.to(DEV), copies.to(DEV))
    assert alpha.shape == o.shape and new_ls.shape == ls.shape and alpha.dtype == new_ls.dtype == torch.float32
    alpha, new_ls = alpha.cpu().numpy().astype(np.float64), new_ls.cpu().numpy().astype(np.float64)
    print("largest |alpha_logit - ref| / (tol (1 + |ref|)):",
          float((np.abs(alpha - want_alpha) / (VALUE_TOL * (1 + np.abs(want_alpha)))).max()))
    print("largest |log_scaling - ref| / (tol (1 + |ref|)):",
          float((np.abs(new_ls - want_ls) / (VALUE_TOL * (1 + np.abs(want_ls)))).max()))
    assert np.isfinite(alpha).all() and np.isfinite(new_ls).all()  # o = 1.0 included: the clamp
    np.testing.assert_allclose(alpha, want_alpha, rtol=VALUE_TOL, atol=VALUE_TOL)
    np.testing.assert_allclose(new_ls, want_ls, rtol=VALUE_TOL, atol=VALUE_TOL)
    # copies above 50 saturate at 51 rows
    at = [i for i, c in enumerate(copies.tolist()) if c >= 50]
    for i in range(0, len(at), 3):
        assert alpha[at[i]] == alpha[at[i + 1]] == alpha[at[i + 2]]
    # the (N, 1) form of opacity, and rows that were not drawn among the drawn ones
    mixed = copies.clone()
    mixed[::2] = 0
    alpha2, ls2 = gs.relocation_values(o.view(-1, 1).to(DEV), ls.to(DEV), mixed.to(DEV))
    assert alpha2.shape == (o.shape[0], 1)
    drawn = (mixed > 0).numpy()
    assert np.array_equal(alpha2.cpu().numpy().reshape(-1)[drawn], alpha.astype(np.float32)[drawn])
    assert np.array_equal(ls2.cpu().numpy()[drawn], new_ls.astype(np.float32)[drawn])


# --------------------------------------------------------------------------------------------------------- perturb
def perturb_scene(n, seed):
    """opacities over 1e-4 .. 0.1 (gate 0.5 .. 1e-4) for 60 % of the rows, 0.5 .. 0.9999 (gate 1e-22 .. exactly 0) for
    the rest; anisotropic scales over 1e-3 .. 1e1; unnormalised rotations"""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n, generator=g, dtype=torch.float64)
    low = torch.exp(math.log(1e-4) + u * (math.log(0.1) - math.log(1e-4)))
    high = 0.5 + 0.4999 * torch.rand(n, generator=g, dtype=torch.float64)
    opacity = torch.where(torch.rand(n, generator=g) < 0.6, low, high)
    if n > 8:
        opacity[:4] = torch.tensor([1e-4, 0.005, 0.1, 0.5], dtype=torch.float64)
        opacity[6:8] = torch.tensor([0.95, 0.9999], dtype=torch.float64)
    table = dict(position=torch.randn(n, 3, generator=g) * 5,
                 log_scaling=torch.rand(n, 3, generator=g) * (math.log(1e1) - math.log(1e-3)) + math.log(1e-3),
                 rotation=torch.randn(n, 4, generator=g) * 3,
                 alpha_logit=torch.log(opacity / (1 - opacity)).float().view(n, 1))
    if n > 8:
        table["position"][5] = torch.tensor([-0.0, 0.0, 1.0])
    return table, torch.randn(n, 3, generator=g)


@pytest.mark.parametrize("n", (1, 65, 20011))
def test_perturb_against_float64(n):
    table, noise = perturb_scene(n, seed=n)
    lr, noise_lr = 1e-5, 5e5
    scale = float(np.float32(lr * noise_lr))
    x0 = float(np.float32(0.995))  # the kernel's argument is a float
    d_ref, gate, exponent = reference_perturb(table["log_scaling"].numpy(), table["rotation"].numpy(),
                                              table["alpha_logit"].numpy(), noise.numpy(), scale, 100.0, x0)
    dev = {name: t.to(DEV) for name, t in table.items()}
    before = dev["position"].clone()
    assert gs.perturb(dev, lr, noise=noise.to(DEV), noise_lr=noise_lr) is None
    for name in ("log_scaling", "rotation", "alpha_logit"):
        assert same_bits(dev[name].cpu(), table[name]), name
    d = (dev["position"].double() - before.double()).cpu().numpy()
    first, second = perturb_bound(table["log_scaling"].numpy(), noise.numpy(), table["position"].numpy(), gate, scale)
    err = np.abs(d - d_ref).max(axis=1)
    moved = first > 0
    # what the 1e-4 allows, used: the error less the position's own rounding, over the first term
    used = np.maximum(err - second, 0)[moved] / first[moved]
    print(f"n = {n}: largest |d - d_ref| / bound = {float((err / (first + second)).max()):.3g}; "
          f"largest (|d - d_ref| - 2^-23 |p|) / (1e-4 scale g max(s^2) |noise|) = {float(used.max(initial=0)):.3g}")
    assert (err <= first + second).all()
    if n > 8:
        assert float(np.abs(d[:3]).max()) > 0  # the open rows did move
    # a gate that is zero in float32 (its exponent is far below expf's range): the position bits stay
    closed = torch.from_numpy(exponent < -90.0)
    assert n < 65 or int(closed.sum()) >= max(2, n // 50)
    assert same_bits(dev["position"].cpu()[closed], table["position"][closed])
    # zero noise keeps every bit, -0.0 included
    dev["position"].copy_(before)
    gs.perturb(dev, lr, noise=torch.zeros(n, 3, device=DEV))
    assert same_bits(dev["position"], before)


def test_perturb_accepts_the_three_containers():
    table, noise = perturb_scene(500, seed=9)
    dev = {name: t.to(DEV) for name, t in table.items()}
    want = {name: t.clone() for name, t in dev.items()}
    gs.perturb(want, 1e-5, noise=noise.to(DEV))
    feature = torch.zeros(500, 3, device=DEV)
    g3d = gs.Gaussians3D(**{name: t.clone() for name, t in dev.items()}, feature=feature)
    gs.perturb(g3d, 1e-5, noise=noise.to(DEV))
    assert same_bits(g3d.position, want["position"])
    params = ParameterClass({**{name: t.clone() for name, t in dev.items()}, "feature": feature},
                            {name: dict(lr=1e-3) for name in dev}, optimizer=torch.optim.Adam)
    pointer = params.tensors["position"].data_ptr()
    gs.perturb(params, 1e-5, noise=noise.to(DEV))
    assert same_bits(params.tensors["position"].detach(), want["position"])
    assert params.tensors["position"].data_ptr() == pointer and params.tensors["position"].requires_grad
    assert not same_bits(want["position"], dev["position"])
    empty = {name: t[:0] for name, t in dev.items()}
    gs.perturb(empty, 1e-5)  # an empty table is a no-op
    gs.perturb(dev, 1e-5)    # the default noise
    assert bool(torch.isfinite(dev["position"]).all())


# ------------------------------------------------------------------------------------------------ relocate and grow
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


def render(params, cam, cfg):
    g = gs.Gaussians3D(**{name: params.tensors[name] for name in GROUPS}, batch_size=params.batch_size)
    return gs.render_gaussians(g, cam, cfg, use_sh=True)


def train_step(params, cam, target, fractional, cfg=RasterConfig(compute_visibility=True)):
    params.zero_grad()
    r = render(params, cam, cfg)
    loss = losses.photometric_loss(r.image, target)
    loss.backward()
    # only the rows that were seen: a row with fresh (zero) optimizer state that is listed with visibility 0 has
    # total_weight 0, and the visibility-aware bias correction sqrt(1 - b2^0) / (1 - b1^0) is 0 / 0
    seen = r.point_visibility > 0
    if fractional:
        params.step(indexes=r.points_in_view[seen], weight=r.point_visibility[seen].clamp(0, 1))
    else:
        params.step(indexes=r.points_in_view[seen], visibility=r.point_visibility[seen])
    return float(loss.detach())


@pytest.fixture(scope="module", params=["VisibilityAwareAdam", "FractionalLaProp"])
def trained(request):
    """a ParameterClass over 1500 rows after three real steps (never changed: the tests work on copies)"""
    n = 1500
    g, cam = sh_scene(n, seed=21)
    optimizer = VisibilityAwareAdam if request.param == "VisibilityAwareAdam" else FractionalLaProp
    params = ParameterClass(dict(g.items()), GROUPS, optimizer=optimizer)
    target = torch.rand(cam.image_size[1], cam.image_size[0], 3, generator=torch.Generator().manual_seed(5)).to(DEV)
    for _ in range(3):
        train_step(params, cam, target, fractional=optimizer is FractionalLaProp)
    params.zero_grad()
    assert all(len(table) >= 2 for table in params.tensor_state.values()) and len(params.tensor_state) == 5
    return params


def copy_of(params):
    return params.apply(lambda t: t.detach().clone())


def arrays(params):
    """(tensors with the float32 sigmoid as 'opacity', state) on the CPU as numpy arrays"""
    tensors = {name: t.detach().cpu().numpy().copy() for name, t in params.tensors.items()}
    tensors["opacity"] = torch.sigmoid(params.tensors["alpha_logit"].detach()).reshape(-1).cpu().numpy()
    state = {name: {key: t.cpu().numpy().copy() for key, t in table.items()}
             for name, table in params.tensor_state.items()}
    return tensors, state


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def assert_table_matches(params, want, want_state, corrected):
    """every column byte for byte, except alpha_logit / log_scaling in the `corrected` rows: the float64 values"""
    for name, t in params.tensors.items():
        got = t.detach().cpu().numpy()
        if name in ("alpha_logit", "log_scaling"):
            rows = corrected
            np.testing.assert_allclose(got[rows].astype(np.float64), want[name][rows], rtol=VALUE_TOL, atol=VALUE_TOL,
                                       err_msg=name)
            assert np.array_equal(raw(got[~rows]), raw(want[name][~rows].astype(np.float32))), name
        else:
            assert got.dtype == want[name].dtype and np.array_equal(raw(got), raw(want[name])), name
    state = params.tensor_state
    assert sorted(state) == sorted(want_state)
    for name, table in want_state.items():
        assert sorted(state[name]) == sorted(table), name
        for key, t in table.items():
            assert np.array_equal(raw(state[name][key].cpu().numpy()), raw(t)), (name, key)


def dead_masks(n):
    g = torch.Generator().manual_seed(31)
    none, every = torch.zeros(n, dtype=torch.bool), torch.ones(n, dtype=torch.bool)
    but_one = every.clone()
    but_one[n // 3] = False
    return {"none": none, "some": torch.rand(n, generator=g) < 0.2, "all_but_one": but_one, "all": every}


@pytest.mark.parametrize("state", ("zero", "sources"))
@pytest.mark.parametrize("case", ("none", "some", "all_but_one", "all"))
def test_relocate_equals_the_composition(trained, case, state):
    params = copy_of(trained)
    n = int(params.batch_size[0])
    dead = dead_masks(n)[case]
    random = random_words(n, seed=41)
    tensors, optimizer_state = arrays(params)
    want, want_state, want_src, want_copies = reference_relocate(tensors, optimizer_state, dead.numpy(),
                                                                 random.numpy(), mode=state)
    objects = {name: t for name, t in params.tensors.items()}
    pointers = {name: t.data_ptr() for name, t in params.tensors.items()}
    state_pointers = {(name, key): t.data_ptr() for name, table in params.tensor_state.items()
                      for key, t in table.items()}
    result = gs.relocate(params, dead.to(DEV), random=random.to(DEV), state=state)
    assert isinstance(result, gs.Relocation)
    assert result.src_of.dtype == torch.int32 and result.copies.dtype == torch.int32
    assert np.array_equal(result.src_of.cpu().numpy(), want_src)
    assert np.array_equal(result.copies.cpu().numpy(), want_copies)
    if case == "some":
        assert want_copies.max() >= 2 and (want_src[dead.numpy()] != np.arange(n)[dead.numpy()]).all()
    if case == "all_but_one":
        assert want_copies[n // 3] == n - 1 and (want_src == n // 3).all()  # the correction saturates at 51
    corrected = (want_copies > 0)[want_src]
    assert_table_matches(params, want, want_state, corrected)
    # in place: the same tensors at the same addresses, the same number of rows
    assert int(params.batch_size[0]) == n
    for name, t in params.tensors.items():
        assert t is objects[name] and t.data_ptr() == pointers[name] and t.requires_grad and t.is_leaf, name
    for name, table in params.tensor_state.items():
        for key, t in table.items():
            assert t.data_ptr() == state_pointers[(name, key)], (name, key)
    # rows neither dead nor drawn: bit-unchanged in every table
    untouched = ~dead.numpy() & (want_copies == 0)
    for name, t in params.tensors.items():
        assert np.array_equal(raw(t.detach().cpu().numpy()[untouched]), raw(tensors[name][untouched])), name
    for name, table in params.tensor_state.items():
        for key, t in table.items():
            assert np.array_equal(raw(t.cpu().numpy()[untouched]), raw(optimizer_state[name][key][untouched]))
    if case in ("none", "all"):  # nothing to move, or nothing to move onto: nothing changes
        assert (want_src == np.arange(n)).all() and not want_copies.any()
        for name, t in params.tensors.items():
            assert same_bits(t.detach(), trained.tensors[name].detach()), name
        for name, table in params.tensor_state.items():
            for key, t in table.items():
                assert same_bits(t, trained.tensor_state[name][key]), (name, key)
    # the optimizer still steps the relocated table
    assert params.optimizer.state[params.tensors["position"]] is not None


def test_relocate_columns_the_kernel_cannot_take():
    """a bool column, 6-byte rows and a strided column go through torch, with the same result"""
    n = 700
    g = torch.Generator().manual_seed(3)
    wide = torch.randn(n, 5, generator=g).to(DEV)
    columns = dict(alpha_logit=torch.randn(n, 1, generator=g).to(DEV), log_scaling=torch.randn(n, 3, generator=g).to(DEV),
                   flag=(torch.rand(n, generator=g) < 0.5).to(DEV),
                   half=torch.randint(-9, 9, (n, 3), generator=g, dtype=torch.int16).to(DEV),
                   wide=torch.randn(n, 40, generator=g).to(DEV))
    params = ParameterClass(columns, dict(alpha_logit=dict(lr=1e-2), log_scaling=dict(lr=1e-3)),
                            optimizer=torch.optim.Adam)
    params.tensors["strided"] = wide[:, :3]
    rest = wide[:, 3:].clone()
    before = {name: t.detach().clone() for name, t in params.tensors.items()}
    dead = torch.rand(n, generator=g) < 0.3
    result = gs.relocate(params, dead.to(DEV), random=random_words(n, 8).to(DEV))
    src_of = result.src_of.long()
    assert bool((src_of[dead.to(DEV)] != torch.arange(n, device=DEV)[dead.to(DEV)]).all())
    for name in ("flag", "half", "wide", "strided"):
        assert same_bits(params.tensors[name].detach().contiguous(), before[name][src_of].contiguous()), name
    assert same_bits(wide[:, 3:].contiguous(), rest)  # the strided column's neighbours in memory


def test_grow_appends_corrected_copies(trained):
    n = int(trained.batch_size[0])
    count = 300
    random = random_words(count, seed=51)
    tensors, optimizer_state = arrays(trained)
    want, want_state, want_src, want_copies = reference_grow(tensors, optimizer_state, random.numpy())
    grown = gs.grow(trained, count, random=random.to(DEV))
    assert grown is not trained and int(grown.batch_size[0]) == n + count and int(trained.batch_size[0]) == n
    assert want_copies.max() >= 2 and int(want_copies.sum()) == count
    corrected = (want_copies > 0)[want_src]
    assert_table_matches(grown, want, want_state, corrected)
    for name, t in grown.tensors.items():
        assert t.requires_grad and t.is_leaf, name
        # the first N rows: byte-equal, except the corrected sources
        kept = ~corrected[:n]
        assert same_bits(t.detach()[:n][torch.from_numpy(kept).to(DEV)],
                         trained.tensors[name].detach()[torch.from_numpy(kept).to(DEV)]), name
    for name, table in grown.tensor_state.items():
        for key, t in table.items():
            assert same_bits(t[:n], trained.tensor_state[name][key]), (name, key)  # the sources keep their state
            assert not bool(t[n:].any()), (name, key)                               # the new rows start at zero
    assert grown.parameter_groups == trained.parameter_groups
    # the source table is untouched
    for name, t in trained.tensors.items():
        assert np.array_equal(raw(t.detach().cpu().numpy()), raw(tensors[name])), name
    # max_rows clips the count; nothing to add returns the same object
    clipped = gs.grow(trained, count, random=random[:100].to(DEV), max_rows=n + 100)
    assert int(clipped.batch_size[0]) == n + 100
    assert np.array_equal(clipped.tensors["position"].detach().cpu().numpy()[n:],
                          tensors["position"][reference_sample(tensors["opacity"], random[:100].numpy())[0]])
    assert gs.grow(trained, 0) is trained and gs.grow(trained, count, max_rows=n) is trained
    assert gs.grow(trained, count, max_rows=n - 5) is trained
    assert int(gs.grow(trained, 7).batch_size[0]) == n + 7  # the default random words


# ------------------------------------------------------------------------------------------------------ a short loop
def test_training_loop_with_the_mcmc_strategy():
    n, cap = 2000, 2300
    g, cam = sh_scene(n, seed=61)
    g.alpha_logit[::10] = -6.0  # opacity 0.0025: a tenth of the rows is dead from the start
    groups = {name: dict(options, lr=2e-2 if name in ("feature", "alpha_logit") else options["lr"])
              for name, options in GROUPS.items()}
    params = ParameterClass(dict(g.items()), groups, optimizer=VisibilityAwareAdam)
    # the target: the same kind of scene from another seed, so that there is something to fit
    other, _ = sh_scene(n, seed=62)
    with torch.no_grad():
        target = gs.render_gaussians(other, cam, RasterConfig(), use_sh=True).image.clamp(0, 1)
    torch.manual_seed(63)
    sizes, first, last = [n], None, None
    for it in range(1, 25):
        last = train_step(params, cam, target, fractional=False)
        first = last if first is None else first
        assert math.isfinite(last)
        gs.perturb(params, params.learning_rates["position"], noise_lr=10.0)
        if it % 6 == 0:
            rows = int(params.batch_size[0])
            opacity = torch.sigmoid(params.tensors["alpha_logit"].detach()).reshape(-1)
            dead = opacity < 0.005
            moved = gs.relocate(params, dead)
            assert int(params.batch_size[0]) == rows and moved.src_of.shape == (rows,)
            if it == 6:
                assert bool(dead.any()) and bool((moved.src_of[dead].long() != dead.nonzero().flatten()).all())
            params = gs.grow(params, int(0.05 * rows), max_rows=cap)
            sizes.append(int(params.batch_size[0]))
        for name, t in params.tensors.items():
            assert bool(torch.isfinite(t.detach()).all()), (it, name)
        for name, table in params.tensor_state.items():
            for key, t in table.items():
                assert bool(torch.isfinite(t).all()), (it, name, key)
    assert sizes == [2000, 2100, 2205, 2300, 2300]
    assert last < first, (first, last)
