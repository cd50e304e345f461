"""HIP path vs CPU oracle on the same seeded inputs (run with -m gpu on an MI355X).
Integer stages (tile decisions, sort keys, order, ranges, scans) are compared bit for bit;
floating-point stages within the tolerances stated in parity_util.py."""
import numpy as np
import pytest
import torch

import config_cases as cc
import parity_util as pu
from golden_util import load_cases, projection_cases, sh_cases
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import taichi_gaussian_rasterizer_amd as gs  # noqa: E402
from taichi_gaussian_rasterizer_amd import RasterConfig, scenes  # noqa: E402
from taichi_gaussian_rasterizer_amd.mapper.tile_mapper import map_to_tiles_reference_stages  # noqa: E402
from taichi_gaussian_rasterizer_amd.perspective import projection as hip_proj  # noqa: E402

DEV = "cuda:0"


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x)) if not isinstance(x, torch.Tensor) else x
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV).contiguous()


# ------------------------------------------------------------------------------------ mapper
MAPPER_CASES = [(0, 500, (320, 200), 16, False), (1, 2000, (257, 131), 16, False), (2, 300, (64, 64), 8, True),
                (3, 50, (100, 40), 32, False), (4, 20000, (640, 360), 16, False), (5, 3000, (96, 96), 16, True),
                (6, 1, (16, 16), 16, False), (7, 5000, (40, 24), 8, False), (8, 3000, (48, 32), 16, False),
                (9, 12000, (64, 48), 16, False)]


@pytest.mark.parametrize("seed,n,size,tile,depth16", MAPPER_CASES)
def test_mapper_bit_exact(seed, n, size, tile, depth16):
    _mapper_bit_exact(seed, n, size, RasterConfig(tile_size=tile), depth16)


@pytest.mark.parametrize("depth16", [False, True])
@pytest.mark.parametrize("tile", [8, 16, 32])
@pytest.mark.parametrize("thr", [1e-4, 1.0 / 255.0, 0.05, 0.3])
def test_mapper_bit_exact_at_other_thresholds(thr, tile, depth16):
    """the tile query's extent is sqrt(2 ln(alpha / thr)) through the deterministic ln and sqrt (map_query.h): from
    r ~ 4.3 sigma at 1e-4 to opacities below the threshold (no tile at all) at 0.3"""
    cfg = RasterConfig(tile_size=tile, alpha_threshold=thr)
    k = _mapper_bit_exact(1, 2000, (257, 131), cfg, depth16)
    k_default = orc.map_to_tiles(*pu.make_2d_scene(1, 2000, (257, 131), scale_factor=0.7, alpha_range=(0.001, 1.0))[:2],
                                 (257, 131), orc.OracleConfig.of(RasterConfig(tile_size=tile)))[0].shape[0]
    assert (k == k_default) == (thr == 1.0 / 255.0), "the threshold must change the overlap count"


def _mapper_bit_exact(seed, n, size, cfg, depth16):
    g2d, depth, _ = pu.make_2d_scene(seed, n, size, scale_factor=0.7, alpha_range=(0.001, 1.0))
    o2p_ref, ranges_ref, keys_ref = orc.map_to_tiles(g2d, depth, size, orc.OracleConfig.of(cfg), depth16, return_keys=True)
    for fn in (gs.map_to_tiles, map_to_tiles_reference_stages):
        o2p, ranges, keys = fn(dev(g2d), dev(depth), size, cfg, use_depth16=depth16, return_keys=True)
        torch.cuda.synchronize()
        assert o2p.dtype == torch.int32 and ranges.dtype == torch.int32
        assert tuple(ranges.shape) == ranges_ref.shape
        assert (pu.to_np(ranges) == ranges_ref).all(), f"{fn.__name__}: tile ranges differ"
        assert (pu.to_np(o2p) == o2p_ref).all(), f"{fn.__name__}: overlap order differs"
        assert (pu.to_np(keys).view(np.uint64) == keys_ref).all(), f"{fn.__name__}: sort keys differ"
    return int(o2p_ref.shape[0])


@pytest.mark.parametrize("n", [600, 1500, 4000, 7000, 9000])
def test_mapper_crowded_tile(n):
    """one tile holding more splats than the wave rank sort covers (512): workgroup merge sort in LDS up to 8192,
    in-place global-memory bitonic network beyond"""
    _mapper_crowded_tile(n, RasterConfig())


def test_mapper_crowded_tile_at_a_low_threshold():
    _mapper_crowded_tile(1500, RasterConfig(alpha_threshold=1e-4))


def _mapper_crowded_tile(n, cfg):
    torch.manual_seed(0)
    g2d = torch.cat([torch.rand(n, 2) * 14 + 1, torch.tensor([[1.0, 0.0]]).expand(n, 2), torch.rand(n, 2) + 0.5,
                     torch.rand(n, 1) * 0.5 + 0.3], 1).float()
    depth = torch.rand(n, 1)
    o2p_ref, ranges_ref = orc.map_to_tiles(g2d, depth, (16, 16), orc.OracleConfig.of(cfg))
    o2p, ranges = gs.map_to_tiles(dev(g2d), dev(depth), (16, 16), cfg)
    assert (pu.to_np(ranges) == ranges_ref).all() and (pu.to_np(o2p) == o2p_ref).all()


def _region_count(tiles_x, tiles_y):
    """the mapper's region grid (csrc/mapper.hip: make_grid): the smallest power-of-two edge >= 8 tiles that keeps the
    region count <= 1024"""
    edge = 8
    while -(-tiles_x // edge) * -(-tiles_y // edge) > 1024:
        edge *= 2
    return -(-tiles_x // edge) * -(-tiles_y // edge)


def test_mapper_scan_path_binning_at_its_smallest_size():
    """The binning pass reserves its places with returning atomics up to 2^16 (workgroup, region) pairs and with the two
    scan launches (region_part_scan_kernel, region_scan_kernel) beyond: 65 workgroups of 1024 Gaussians x 1024 regions is
    the smallest standalone call that takes the scans."""
    tile, size, n = 8, (2048, 2048), 64 * 1024 + 1
    regions = _region_count(size[0] // tile, size[1] // tile)
    assert regions == 1024 and -(-n // 1024) * regions > 65536
    rng = np.random.default_rng(3)
    mean = rng.uniform(0.0, 1.0, (n, 2)) * np.array(size, np.float64)
    angle = rng.uniform(0.0, 2.0 * np.pi, n)
    sigma = rng.uniform(0.5, 3.0, (n, 2))
    alpha = rng.uniform(0.05, 0.9, (n, 1))
    g2d = np.concatenate([mean, np.cos(angle)[:, None], np.sin(angle)[:, None], sigma, alpha], 1).astype(np.float32)
    depth = rng.random((n, 1)).astype(np.float32)
    cfg = RasterConfig(tile_size=tile)
    o2p_ref, ranges_ref = orc.map_to_tiles(g2d, depth, size, orc.OracleConfig.of(cfg))
    o2p, ranges = gs.map_to_tiles(dev(g2d), dev(depth), size, cfg)
    assert (pu.to_np(ranges) == ranges_ref).all(), "tile ranges differ"
    assert (pu.to_np(o2p) == o2p_ref).all(), "overlap order differs"


@pytest.mark.parametrize("depth16", [False, True])
@pytest.mark.parametrize("lo,step", [(40, 6), (40, 15)])
def test_mapper_clustered_depths_through_every_row_count(lo, step, depth16):
    """Tile t of a 8 x 4 grid holds exactly lo + step t splats, on three depth values: the wave sort's bucket sort gives
    up on a bin of more than 40 keys (tile_sort.hip: BIN_LIMIT) and the rank sort runs, at every row count (64 keys per
    row) of tile_rank_sort_kernel<4> ((40, 6): up to 226 splats) and <8> ((40, 15): up to 505).  Ties come out in
    ascending Gaussian index."""
    tile, size, tiles_x, num_tiles = 16, (128, 64), 8, 32
    counts = lo + step * np.arange(num_tiles)
    n = int(counts.sum())
    rng = np.random.default_rng(11)
    t = np.repeat(np.arange(num_tiles), counts)
    origin = np.stack([(t % tiles_x) * tile, (t // tiles_x) * tile], 1).astype(np.float64)
    mean = origin + 5.0 + 6.0 * rng.random((n, 2))
    alpha = rng.uniform(0.3, 0.9, (n, 1))
    depth = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), (n, 1))
    g2d = np.concatenate([mean, np.tile([1.0, 0.0], (n, 1)), np.full((n, 2), 0.4), alpha], 1).astype(np.float32)
    perm = rng.permutation(n)  # index order is not tile order
    g2d, depth = g2d[perm], depth[perm]
    cfg = RasterConfig(tile_size=tile)
    o2p_ref, ranges_ref, keys_ref = orc.map_to_tiles(g2d, depth, size, orc.OracleConfig.of(cfg), depth16,
                                                     return_keys=True)
    flat = ranges_ref.reshape(num_tiles, 2)
    assert (flat[:, 1] - flat[:, 0] == counts).all(), "the layout's tile populations"
    most_shared = {}  # row count -> most entries on one depth value in some tile of that row count
    for a, b in flat:
        rows = -(-int(b - a) // 64)
        shared = int(np.unique(depth[o2p_ref[a:b], 0], return_counts=True)[1].max())
        most_shared[rows] = max(most_shared.get(rows, 0), shared)
    max_rows = -(-int(counts.max()) // 64)
    assert max_rows == (4 if step == 6 else 8)
    assert all(most_shared[rows] > 40 for rows in range(2, max_rows + 1)), most_shared
    o2p, ranges, keys = gs.map_to_tiles(dev(g2d), dev(depth), size, cfg, use_depth16=depth16, return_keys=True)
    assert (pu.to_np(ranges) == ranges_ref).all(), "tile ranges differ"
    assert (pu.to_np(o2p) == o2p_ref).all(), "overlap order differs"
    assert (pu.to_np(keys).view(np.uint64) == keys_ref).all(), "sort keys differ"


def test_mapper_empty_and_culled():
    cfg = RasterConfig()
    o2p, ranges = gs.map_to_tiles(torch.zeros((0, 7), device=DEV), torch.zeros((0, 1), device=DEV), (40, 30), cfg)
    assert o2p.shape == (0,) and tuple(ranges.shape) == (2, 3, 2) and int(ranges.abs().sum()) == 0
    g = torch.tensor([[20., 15., 1., 0., 3., 3., 0.001], [-500., -500., 1., 0., 2., 2., 0.9]], device=DEV)
    o2p, ranges = gs.map_to_tiles(g, torch.tensor([[0.5], [0.2]], device=DEV), (40, 30), cfg)
    ref_o2p, ref_ranges = orc.map_to_tiles(g.cpu(), np.array([[0.5], [0.2]], np.float32), (40, 30))
    assert (pu.to_np(o2p) == ref_o2p).all() and (pu.to_np(ranges) == ref_ranges).all()


def test_map_prepare_mirrors_its_counts_to_pinned_host_memory():
    """gs_map_prepare(counts_host): the scan kernel stores {K, fullest tile, overflow, heavy tiles, *v_dev} into pinned
    host words itself -- what the fused frame waits for instead of a device-to-host copy"""
    import ctypes
    from taichi_gaussian_rasterizer_amd import _native as nv
    torch.manual_seed(3)
    n, size = 5000, (320, 200)
    g2d = torch.cat([torch.rand(n, 1) * size[0], torch.rand(n, 1) * size[1], torch.tensor([[1.0, 0.0]]).expand(n, 2),
                     torch.rand(n, 2) * 6 + 0.5, torch.rand(n, 1) * 0.6 + 0.3], 1).float()
    depth = torch.rand(n, 1)
    cfg = RasterConfig()
    o2p_ref, ranges_ref = orc.map_to_tiles(g2d, depth, size, orc.OracleConfig.of(cfg))
    lib = nv.lib()
    tiles = ranges_ref.reshape(-1, 2).shape[0]
    pts = dev(g2d)
    ranges = torch.empty((tiles, 2), dtype=torch.int32, device=DEV)
    counts = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    order = torch.empty((tiles,), dtype=torch.int32, device=DEV)
    v_dev = torch.tensor([n - 100], dtype=torch.int32, device=DEV)   # live rows < capacity
    host = torch.full((5,), -7, dtype=torch.int32).pin_memory()
    nbytes = lib.gs_map_scratch_bytes(n, tiles)
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    for k_cap in (0, 1000):  # unbounded, then a capacity that overflows
        nv.check(lib.gs_map_prepare(n, nv.ptr(v_dev), nv.ptr(pts), size[0], size[1], nv.make_config(cfg), k_cap,
                                    nv.ptr(ranges), nv.ptr(counts), nv.ptr(host), nv.ptr(order), None, nv.ptr(scratch),
                                    nbytes, nv.stream()), "gs_map_prepare")
        torch.cuda.synchronize()
        assert host[:4].tolist() == counts.tolist() and int(host[4]) == n - 100
        assert int(host[2]) == (1 if k_cap else 0)
    o2p_live, _ = orc.map_to_tiles(g2d[:n - 100], depth[:n - 100], size, orc.OracleConfig.of(cfg))
    assert int(host[0]) == o2p_live.shape[0]


def test_device_sqrt_and_log_are_the_host_ones_bit_for_bit():
    """the mapper's integer decisions are f32 geometry: every operation must round identically on gfx950 and on the
    host.  sqrt: hipcc's __fsqrt_rn is the 1-ulp v_sqrt_f32 (rounds 1-2 used it; C5 at full size found the splat it
    misplaces) -- gs_det_sqrtf must equal IEEE sqrt on every input; ln: gs_det_logf against the oracle's build of the
    same source."""
    from taichi_gaussian_rasterizer_amd import _native as nv
    rng = np.random.default_rng(0)
    x = np.concatenate([np.exp(rng.uniform(-80, 80, 6_000_000)), rng.uniform(0, 4, 2_000_000),
                        rng.uniform(1, 1e6, 2_000_000), [0.0, 1.0, 4.0, 2.0 ** -100, 2.0 ** -126, 3.0e38]]).astype(np.float32)
    xd = dev(x)
    s_out, l_out = torch.empty_like(xd), torch.empty_like(xd)
    nv.check(nv.lib().gs_selftest_detmath(x.shape[0], nv.ptr(xd), nv.ptr(s_out), nv.ptr(l_out), nv.stream()),
             "gs_selftest_detmath")
    got = pu.to_np(s_out)
    want = np.sqrt(x)  # IEEE-754 correctly rounded
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, f"{bad.size} of {x.shape[0]} square roots differ, e.g. x = {x[bad[:3]]}"
    sub_ = np.concatenate([rng.choice(x.shape[0] - 6, 20_000, replace=False), [x.shape[0] - 5, x.shape[0] - 4]])
    ref = np.array([orc.lib().orc_det_logf(float(v)) for v in x[sub_]], np.float32)
    assert (pu.to_np(l_out)[sub_].view(np.uint32) == ref.view(np.uint32)).all()


@pytest.mark.parametrize("F,col0,world,v", [(3, 0, 8, 100_000), (5, 2, 3, 777), (12, 0, 64, 5000), (3, 0, 1, 300)])
def test_sparse_exchange_kernels(F, col0, world, v):
    """the three kernels of the sharded frame's sparse exchange against numpy: gs_shard_pack_sparse (entries [row, 7 + F
    words], colour gradients of clamped channels zeroed), gs_shard_add_sparse (one list into the dense rows) and
    gs_shard_merge_sparse (all lists in one pass) -- the latter two must agree BIT FOR BIT (same summation order)"""
    import ctypes
    from taichi_gaussian_rasterizer_amd import _native as nv
    lib = nv.lib()
    rng = np.random.default_rng(F * 100 + world)
    RS = lib.gs_grad_row_floats(F)
    W = 8 + F
    lists, counts = [], []
    for q in range(world):
        m = int(rng.integers(0, max(v // max(world // 2, 1), 2)))
        rows = np.sort(rng.choice(v, size=min(m, v), replace=False)).astype(np.int32)
        grad = rng.standard_normal((v, RS)).astype(np.float32)
        feats = rng.random((v, F)).astype(np.float32)
        feats[rng.random((v, F)) < 0.2] = 1.0          # clamped channels
        ent = torch.empty((max(rows.shape[0], 1) + 3, W), dtype=torch.float32, device=DEV)  # + padding rows
        ent.view(torch.int32)[:, 0] = -1
        rows_d, grad_d, feats_d = dev(rows), dev(grad), dev(feats)  # named: the buffers must outlive the launch
        nv.check(lib.gs_shard_pack_sparse(rows.shape[0], nv.ptr(rows_d), F, col0, nv.ptr(grad_d),
                                          nv.ptr(feats_d), nv.ptr(ent), nv.stream()), "gs_shard_pack_sparse")
        torch.cuda.synchronize()
        want = np.concatenate([rows.view(np.float32)[:, None], grad[rows, :7 + F]], 1)
        mask = ~((feats[rows] > 0) & (feats[rows] < 1))
        mask[:, :col0] = False
        want[:, 8:][mask] = 0.0
        got = pu.to_np(ent)[:rows.shape[0]]
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), f"pack of list {q}"
        lists.append(ent)
        counts.append(int(rows.shape[0]))
    # list by list
    pf = torch.zeros((v, F - col0), device=DEV)
    pp = torch.zeros((v, 7 + col0), device=DEV)
    for ent, cnt in zip(lists, counts):
        nv.check(lib.gs_shard_add_sparse(cnt + 3, nv.ptr(ent), F, col0, v, nv.ptr(pf), nv.ptr(pp), nv.stream()),
                 "gs_shard_add_sparse")   # the padding rows (id -1) are skipped
    ref_p, ref_f = np.zeros((v, 7 + col0), np.float32), np.zeros((v, F - col0), np.float32)
    for ent, cnt in zip(lists, counts):
        e = pu.to_np(ent)[:cnt]
        ids = e[:, 0].view(np.int32)
        ref_p[ids] += e[:, 1:8 + col0]
        ref_f[ids] += e[:, 8 + col0:]
    assert (pu.to_np(pp) == ref_p).all() and (pu.to_np(pf) == ref_f).all()
    # all at once: every row written (the buffers start as garbage), same bits
    mf = torch.full((v, F - col0), float("nan"), device=DEV)
    mp_ = torch.full((v, 7 + col0), float("nan"), device=DEV)
    ptrs = (ctypes.c_void_p * world)(*[e.data_ptr() for e in lists])
    cnts = (ctypes.c_int64 * world)(*counts)
    tmp_bytes = 4 * world * (-(-v // 256) + 1)
    tmp = torch.empty((tmp_bytes,), dtype=torch.uint8, device=DEV)
    nv.check(lib.gs_shard_merge_sparse(world, ptrs, cnts, F, col0, v, nv.ptr(mf), nv.ptr(mp_), None, nv.ptr(tmp),
                                       tmp_bytes, nv.stream()), "gs_shard_merge_sparse")
    assert torch.equal(mp_, pp) and torch.equal(mf, pf)
    # with a row range only the tiles that meet it are written (sharded gradients read nothing else)
    lo, hi = v // 3, v // 3 + max(v // 4, 1)
    rng_d = torch.tensor([lo, hi], dtype=torch.int32, device=DEV)
    mf.fill_(float("nan")); mp_.fill_(float("nan"))
    nv.check(lib.gs_shard_merge_sparse(world, ptrs, cnts, F, col0, v, nv.ptr(mf), nv.ptr(mp_), nv.ptr(rng_d),
                                       nv.ptr(tmp), tmp_bytes, nv.stream()), "gs_shard_merge_sparse")
    assert torch.equal(mp_[lo:hi], pp[lo:hi]) and torch.equal(mf[lo:hi], pf[lo:hi])
    t0, t1 = (lo // 256) * 256, min(-(-hi // 256) * 256, v)
    assert bool(torch.isnan(mp_[:t0]).all()) and bool(torch.isnan(mp_[t1:]).all())


def test_sh_forward_over_a_row_list():
    """gs_sh_fwd_rows (the sharded frame's colour stage: exactly the rows of the mapper's touched list) writes the same
    bits as gs_sh_fwd for the listed rows and leaves every other row alone"""
    from taichi_gaussian_rasterizer_amd import _native as nv
    lib = nv.lib()
    n, v, C, deg = 5000, 4200, 3, 3
    gen = torch.Generator().manual_seed(3)
    params = dev(torch.randn(n, C, 16, generator=gen) * 0.3)
    pos = dev(torch.randn(n, 3, generator=gen) * 4)
    indexes = dev(torch.sort(torch.randperm(n, generator=gen)[:v])[0])
    cam = dev(torch.tensor([0.1, -0.2, 0.3]))
    full = torch.empty((v, C), device=DEV)
    nv.check(lib.gs_sh_fwd(v, None, C, deg, nv.ptr(params), nv.ptr(pos), nv.ptr(indexes), nv.ptr(cam), nv.ptr(full), C,
                           nv.stream()), "gs_sh_fwd")
    rows = dev(torch.sort(torch.randperm(v, generator=gen)[:1500])[0].to(torch.int32))
    count = dev(torch.tensor([1200], dtype=torch.int32))       # the list is longer than its live count
    out = torch.full((v, C), -7.0, device=DEV)
    nv.check(lib.gs_sh_fwd_rows(rows.shape[0], nv.ptr(rows), nv.ptr(count), C, deg, nv.ptr(params), nv.ptr(pos),
                                nv.ptr(indexes), nv.ptr(cam), nv.ptr(out), C, nv.stream()), "gs_sh_fwd_rows")
    listed = rows[:1200].long()
    assert torch.equal(out[listed], full[listed])
    mask = torch.ones(v, dtype=torch.bool, device=DEV)
    mask[listed] = False
    assert bool((out[mask] == -7.0).all())


def test_hip_lib_cumsum_and_sort():
    rng = np.random.default_rng(0)
    # (1 << 20) + 1: 1025 block sums, the first second round (and carry) of the scan over them
    for n in (1, 2, 1023, 1024, 1025, 100000, 1 << 20, (1 << 20) + 1):
        x = rng.integers(0, 50, n).astype(np.int32)
        out, total = gs.hip_lib.full_cumsum(dev(x))
        ref = np.concatenate([[0], np.cumsum(x.astype(np.int64))])
        assert total == ref[-1] and (pu.to_np(out).astype(np.int64) == ref).all()
    out, total = gs.hip_lib.full_cumsum(torch.zeros((0,), dtype=torch.int32, device=DEV))
    assert total == 0 and out.shape == (1,)
    for n, bits, dt in ((1, (0, 64), np.uint64), (5000, (0, 48), np.uint64), (300000, (0, 48), np.uint64),
                        (70000, (8, 40), np.uint64), (100000, (0, 32), np.uint32), (4097, (0, 20), np.uint32)):
        keys = rng.integers(0, 1 << 62 if dt == np.uint64 else 1 << 32, n, dtype=np.uint64).astype(dt)
        keys[rng.integers(0, n, n // 3)] = keys[0]  # plenty of duplicates: stability is observable
        vals = np.arange(n, dtype=np.int32)
        tdt = torch.int64 if dt == np.uint64 else torch.int32
        k_out, v_out = gs.hip_lib.radix_sort_pairs(dev(keys.view(np.int64 if dt == np.uint64 else np.int32), tdt),
                                                   dev(vals), bits[0], bits[1])
        mask = (1 << (bits[1] - bits[0])) - 1
        order = np.argsort(((keys.astype(np.uint64) >> np.uint64(bits[0])) & np.uint64(mask)), kind="stable")
        assert (pu.to_np(v_out) == vals[order]).all(), f"n={n} bits={bits}"
        assert (pu.to_np(k_out).view(dt) == keys[order]).all()
    with pytest.raises(RuntimeError):
        gs.hip_lib.full_cumsum(torch.zeros(4, device=DEV))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int16])
def test_hip_lib_segmented_sort_pairs(dtype):
    """cuda_lib.segmented_sort_pairs (reference cuda_lib/__init__.py:27,47-56): per-segment ascending sort of signed
    keys, against torch.sort; a gap between segments, an empty segment, one beyond the LDS capacity"""
    gen = torch.Generator().manual_seed(0)
    bounds = [0, 8, 16, 16, 700, 9800, 30000]          # segment s = [bounds[s], bounds[s+1]) except the gap below
    starts = torch.tensor(bounds[:-1], dtype=torch.int64)
    ends = torch.tensor(bounds[1:], dtype=torch.int64)
    ends[0] = 6                                         # items 6, 7 belong to no segment
    n = bounds[-1]
    lim = 30000 if dtype == torch.int16 else 2 ** 31 - 1
    k = torch.randint(-lim, lim, (n,), generator=gen).to(dtype)
    v = torch.arange(n, dtype=torch.int32)
    ko, vo = gs.hip_lib.segmented_sort_pairs(dev(k), dev(v), dev(starts), dev(ends))
    ko, vo = ko.cpu(), vo.cpu()
    for a, b in zip(starts.tolist(), ends.tolist()):
        ref, order = torch.sort(k[a:b].long(), stable=True)
        assert torch.equal(ko[a:b].long(), ref) and torch.equal(vo[a:b].long(), order + a)
    assert torch.equal(ko[6:8], k[6:8]) and torch.equal(vo[6:8], v[6:8])
    with pytest.raises(RuntimeError):
        gs.hip_lib.segmented_sort_pairs(dev(k.long()), dev(v), dev(starts), dev(ends))


# -------------------------------------------------------------------------------- rasterizer
RASTER_CASES = [(0, 40, (8, 8), 8, 3), (1, 300, (64, 48), 16, 3), (2, 500, (50, 37), 16, 1), (3, 64, (33, 17), 8, 2),
                (4, 1000, (96, 64), 32, 3), (5, 4000, (320, 200), 16, 5), (6, 800, (128, 72), 16, 8),
                (7, 300, (48, 48), 16, 12), (8, 20000, (256, 256), 16, 3)]


@pytest.mark.parametrize("seed,n,size,tile,F", RASTER_CASES)
def test_raster_forward_backward(seed, n, size, tile, F):
    g2d, depth, feat = pu.make_2d_scene(seed, n, size, channels=F, scale_factor=0.5)
    cfg = RasterConfig(tile_size=tile)
    ocfg = orc.OracleConfig.of(cfg)
    o2p, ranges = orc.map_to_tiles(g2d, depth, size, ocfg)
    image_ref, alpha_ref, _ = orc.rasterize_with_tiles(g2d, feat, o2p, ranges, size, ocfg)
    g_t, f_t = dev(g2d).requires_grad_(True), dev(feat).requires_grad_(True)
    out = gs.rasterize_with_tiles(g_t, f_t, dev(o2p), dev(ranges.reshape(-1, 2)), size, cfg)
    assert tuple(out.image.shape) == (size[1], size[0], F) and tuple(out.image_weight.shape) == (size[1], size[0])
    proof = pu.flip_proof(g2d, feat, o2p, ranges, size, ocfg)
    pu.assert_pixels_close(out.image, image_ref, "image", flips=proof)
    pu.assert_pixels_close(out.image_weight, alpha_ref, "alpha", flips=proof.weight())
    torch.manual_seed(100 + seed)
    gi = torch.rand(size[1], size[0], F)
    (out.image * dev(gi)).sum().backward()
    # the backward consumes the forward's own image: give the oracle the HIP image so that the only
    # difference measured is the backward kernel
    gg, gf, _ = orc.rasterize_backward(g2d, feat, o2p, ranges, size, pu.to_np(out.image), gi.numpy(), ocfg)
    _, gg64, gf64 = pu.raster_truth(g2d, feat, o2p, ranges, size, ocfg, gi)
    pu.assert_grad_close_vs_truth(g_t.grad, gg, gg64, "grad_gaussians2d")
    pu.assert_grad_close_vs_truth(f_t.grad, gf, gf64, "grad_features")


@pytest.mark.parametrize("heur", [False, True])
def test_raster_extreme_opacities(heur):
    """the lean kernels stage -log2(opacity) and let v_exp_f32 return alpha: opacities at the threshold, at and beyond
    the clamp (0.99) and above 1 (a caller's own 2D splats may carry any value) against the oracle's
    opacity * exp(...) -- forward, backward and (heur) the densification statistics of the MODE 1 kernels"""
    cfg = RasterConfig(compute_point_heuristic=heur)
    thr = cfg.alpha_threshold
    _raster_extreme_opacities(cfg, [thr * (1 - 1e-3), thr * (1 + 1e-3), thr * 1.5, 0.05, 0.5, 0.98, 0.99, 0.995, 1.0,
                                    1.5, 4.0])


@pytest.mark.parametrize("heur", [False, True], ids=["lean", "heur"])
@pytest.mark.parametrize("cid", ["thr_small", "clamp_half", "mixed"])
def test_raster_extreme_opacities_at_other_settings(cid, heur):
    """the ladder rebuilt around the setting's threshold and clamp: just under and over the threshold, at and over the
    clamp, and above 1"""
    cfg = cc.raster_config(cid, 16, compute_point_heuristic=heur)
    thr, cmax = cfg.alpha_threshold, cfg.clamp_max_alpha
    _raster_extreme_opacities(cfg, [thr * (1 - 1e-3), thr * (1 + 1e-3), thr * 1.5, 0.05, 0.5 * cmax, cmax * (1 - 1e-3),
                                    cmax, cmax * (1 + 1e-3), 1.0, 1.5, 4.0], scale_bar=True)


def _raster_extreme_opacities(cfg, vals, scale_bar=False):
    """vals[0] is below the threshold: the rows that carry it must get an exactly zero gradient"""
    heur = cfg.compute_point_heuristic
    size, n, F = (96, 64), 600, 3
    g2d, depth, feat = pu.make_2d_scene(21, n, size, channels=F, scale_factor=0.6)
    vals = np.array(vals, np.float32)
    g2d = pu.to_np(g2d).copy()
    g2d[:, 6] = vals[np.arange(n) % len(vals)]
    ocfg = orc.OracleConfig.of(cfg)
    o2p, ranges = orc.map_to_tiles(g2d, depth, size, ocfg)
    image_ref, alpha_ref, _ = orc.rasterize_with_tiles(g2d, feat, o2p, ranges, size, ocfg)
    g_t, f_t = dev(g2d).requires_grad_(True), dev(feat).requires_grad_(True)
    out = gs.rasterize_with_tiles(g_t, f_t, dev(o2p), dev(ranges.reshape(-1, 2)), size, cfg)
    proof = pu.flip_proof(g2d, feat, o2p, ranges, size, ocfg,
                          bar=cc.raster_bar(cfg, g2d) if scale_bar else pu.FLIP_MARGIN)
    pu.assert_pixels_close(out.image, image_ref, "image", flips=proof)
    pu.assert_pixels_close(out.image_weight, alpha_ref, "alpha", flips=proof.weight())
    gi = torch.rand(size[1], size[0], F, generator=torch.Generator().manual_seed(22))
    (out.image * dev(gi)).sum().backward()
    gg, gf, heur_ref = orc.rasterize_backward(g2d, feat, o2p, ranges, size, pu.to_np(out.image), gi.numpy(), ocfg)
    _, gg64, gf64 = pu.raster_truth(g2d, feat, o2p, ranges, size, ocfg, gi)
    pu.assert_grad_close_vs_truth(g_t.grad, gg, gg64, "grad_gaussians2d")
    pu.assert_grad_close_vs_truth(f_t.grad, gf, gf64, "grad_features")
    assert torch.isfinite(g_t.grad).all() and float(g_t.grad[::len(vals)].abs().max()) == 0.0  # below the threshold
    if heur:
        pu.assert_grad_close(out.point_heuristic, heur_ref, "point_heuristic", tol=1e-3)


@pytest.mark.parametrize("nb", [1, 2, 4])
@pytest.mark.parametrize("seed,n,size,tile,F", [(11, 3000, (200, 120), 16, 3), (12, 2000, (160, 96), 32, 5)])
def test_raster_wave_region_variants(nb, seed, n, size, tile, F, monkeypatch):
    """the rasterizer picks 16x16, 16x8 or 8x8 pixel regions per wave from the grid size (gs_raster_sub_blocks);
    the per-call tuning field GsRasterConfig.tune_wave_sub_blocks forces each variant on the same scene: all must
    agree with the oracle"""
    from taichi_gaussian_rasterizer_amd import _native as nv
    monkeypatch.setitem(nv.TUNING, "wave_sub_blocks", int(nb))
    g2d, depth, feat = pu.make_2d_scene(seed, n, size, channels=F, scale_factor=0.5)
    cfg = RasterConfig(tile_size=tile, compute_visibility=(nb == 2))
    ocfg = orc.OracleConfig.of(cfg)
    o2p, ranges = orc.map_to_tiles(g2d, depth, size, ocfg)
    image_ref, alpha_ref, vis_ref = orc.rasterize_with_tiles(g2d, feat, o2p, ranges, size, ocfg)
    g_t, f_t = dev(g2d).requires_grad_(True), dev(feat).requires_grad_(True)
    out = gs.rasterize_with_tiles(g_t, f_t, dev(o2p), dev(ranges.reshape(-1, 2)), size, cfg)
    proof = pu.flip_proof(g2d, feat, o2p, ranges, size, ocfg)
    pu.assert_pixels_close(out.image, image_ref, "image", flips=proof)
    pu.assert_pixels_close(out.image_weight, alpha_ref, "alpha", flips=proof.weight())
    if cfg.compute_visibility:
        pu.assert_grad_close(out.visibility, vis_ref, "visibility", tol=1e-5)
    gi = torch.rand(size[1], size[0], F, generator=torch.Generator().manual_seed(seed))
    (out.image * dev(gi)).sum().backward()
    gg, gf, _ = orc.rasterize_backward(g2d, feat, o2p, ranges, size, pu.to_np(out.image), gi.numpy(), ocfg)
    _, gg64, gf64 = pu.raster_truth(g2d, feat, o2p, ranges, size, ocfg, gi)
    pu.assert_grad_close_vs_truth(g_t.grad, gg, gg64, "grad_gaussians2d")
    pu.assert_grad_close_vs_truth(f_t.grad, gf, gf64, "grad_features")


@pytest.mark.parametrize("nb", [1, 2, 4])
def test_raster_antialias_gradients_at_scale(nb, monkeypatch):
    """the antialiased pdf (taichi_lib/generic.py:341-404) beyond the reference's 8x8 gradcheck scene: tile 16,
    >= 300 splats in EVERY tile (five or more staging groups per wave, saturation inside the lists), blur_cov = 0 as
    the reference pairs it, all three wave-region shapes -- so the support-box sub-block masks
    (gs_sub_block_mask_antialias) decide for every block of every tile.  Pixels vs the f32 oracle, gradients vs the f32
    oracle with the f64 oracle as yardstick, at the suite's stated bars."""
    from taichi_gaussian_rasterizer_amd import _native as nv
    monkeypatch.setitem(nv.TUNING, "wave_sub_blocks", int(nb))
    size, n, F = (128, 96), 8000, 3
    g2d, depth, feat = pu.make_2d_scene(31, n, size, channels=F, scale_factor=2.0)
    cfg = RasterConfig(antialias=True, blur_cov=0.0)
    ocfg = orc.OracleConfig.of(cfg)
    o2p, ranges = orc.map_to_tiles(g2d, depth, size, ocfg)
    assert int((ranges[..., 1] - ranges[..., 0]).min()) >= 300
    image_ref, alpha_ref, _ = orc.rasterize_with_tiles(g2d, feat, o2p, ranges, size, ocfg)
    g_t, f_t = dev(g2d).requires_grad_(True), dev(feat).requires_grad_(True)
    out = gs.rasterize_with_tiles(g_t, f_t, dev(o2p), dev(ranges.reshape(-1, 2)), size, cfg)
    proof = pu.flip_proof(g2d, feat, o2p, ranges, size, ocfg, bar=pu.AA_FLIP_MARGIN)
    pu.assert_pixels_close(out.image, image_ref, "antialias image", flips=proof)
    pu.assert_pixels_close(out.image_weight, alpha_ref, "antialias weight", flips=proof.weight())
    gi = torch.rand(size[1], size[0], F, generator=torch.Generator().manual_seed(32))
    (out.image * dev(gi)).sum().backward()
    gg, gf, _ = orc.rasterize_backward(g2d, feat, o2p, ranges, size, pu.to_np(out.image), gi.numpy(), ocfg)
    _, gg64, gf64 = pu.raster_truth(g2d, feat, o2p, ranges, size, ocfg, gi)
    pu.assert_grad_close_vs_truth(g_t.grad, gg, gg64, "antialias grad_gaussians2d")
    pu.assert_grad_close_vs_truth(f_t.grad, gf, gf64, "antialias grad_features")
    pu.assert_rows_close(g_t.grad, gg64, "antialias grad_gaussians2d rows", tol=1e-2, frac=0.995)
    pu.assert_rows_close(f_t.grad, gf64, "antialias grad_features rows", tol=1e-2, frac=0.995)


@pytest.mark.parametrize("cfg_kw", [dict(), dict(compute_point_heuristic=True), dict(antialias=True, blur_cov=0.0)])
def test_raster_listed_splats_without_opacity(cfg_kw):
    """rasterize_with_tiles takes the CALLER'S tile lists (function.py:96-127), which may hold splats whose opacity was
    zeroed or masked after map_to_tiles: opacity 0, a subnormal, and values at or below alpha_threshold.  Such a splat
    blends nothing; its gradient row must be exactly zero and finite (the lean backward divides its opacity out of the
    reduced sums), everything else as in the oracle."""
    size, n, F = (96, 64), 500, 3
    g2d, depth, feat = pu.make_2d_scene(41, n, size, channels=F, scale_factor=0.6)
    cfg = RasterConfig(**cfg_kw)
    ocfg = orc.OracleConfig.of(cfg)
    o2p, ranges = orc.map_to_tiles(g2d, depth, size, ocfg)          # lists built with every splat opaque enough
    g2d = pu.to_np(g2d).copy()
    dead = np.array([0.0, 1e-42, cfg.alpha_threshold * 0.5, cfg.alpha_threshold], np.float32)
    g2d[:200, 6] = dead[np.arange(200) % 4]
    assert np.isin(np.arange(200), o2p).all()                       # ... and the dead ones are listed
    image_ref, alpha_ref, _ = orc.rasterize_with_tiles(g2d, feat, o2p, ranges, size, ocfg)
    g_t, f_t = dev(g2d).requires_grad_(True), dev(feat).requires_grad_(True)
    out = gs.rasterize_with_tiles(g_t, f_t, dev(o2p), dev(ranges.reshape(-1, 2)), size, cfg)
    proof = pu.flip_proof(g2d, feat, o2p, ranges, size, ocfg, bar=pu.AA_FLIP_MARGIN if cfg.antialias else pu.FLIP_MARGIN)
    pu.assert_pixels_close(out.image, image_ref, "image", flips=proof)
    gi = torch.rand(size[1], size[0], F, generator=torch.Generator().manual_seed(42))
    (out.image * dev(gi)).sum().backward()
    gg, gf, heur_ref = orc.rasterize_backward(g2d, feat, o2p, ranges, size, pu.to_np(out.image), gi.numpy(), ocfg)
    assert torch.isfinite(g_t.grad).all() and torch.isfinite(f_t.grad).all()
    assert float(g_t.grad[:200].abs().max()) == 0.0 and float(f_t.grad[:200].abs().max()) == 0.0
    assert float(np.abs(gg[:200]).max()) == 0.0
    _, gg64, gf64 = pu.raster_truth(g2d, feat, o2p, ranges, size, ocfg, gi)
    pu.assert_grad_close_vs_truth(g_t.grad, gg, gg64, "grad_gaussians2d")
    pu.assert_grad_close_vs_truth(f_t.grad, gf, gf64, "grad_features")
    if cfg.compute_point_heuristic:
        assert torch.isfinite(out.point_heuristic).all()
        pu.assert_grad_close(out.point_heuristic, heur_ref, "point_heuristic", tol=1e-3)


@pytest.mark.parametrize("seed", range(3))
def test_raster_reference_gradcheck_scene(seed):
    """the reference's own rasterizer test scene (tests/test_rasterizer.py:30-59), f32 vs oracle f64"""
    torch.manual_seed(seed)
    n = torch.randint(1, 50, (1,)).item()
    channels = torch.randint(1, 4, (1,)).item()
    g = scenes.random_2d_gaussians(n, (8, 8), num_channels=channels, scale_factor=1.0, alpha_range=(0.2, 0.8))
    g2d = gs.misc.renderer2d.project_gaussians2d(g) if hasattr(gs, "misc") else None
    from taichi_gaussian_rasterizer_amd.misc.renderer2d import project_gaussians2d
    g2d = project_gaussians2d(g).float()
    for antialias in (False, True):
        cfg = RasterConfig(tile_size=8, pixel_stride=(1, 1), antialias=antialias)
        o2p = np.arange(n, dtype=np.int32)
        ranges = np.array([[0, n]], np.int32)
        image_ref, _, _ = orc.rasterize_with_tiles(g2d.double(), g.feature.double(), o2p, ranges, (8, 8),
                                                   orc.OracleConfig.of(cfg))
        g_t, f_t = dev(g2d).requires_grad_(True), dev(g.feature.float()).requires_grad_(True)
        out = gs.rasterize_with_tiles(g_t, f_t, dev(o2p), dev(ranges), (8, 8), cfg)
        proof = pu.flip_proof(g2d, g.feature.float(), o2p, ranges, (8, 8), orc.OracleConfig.of(cfg),
                              bar=pu.AA_FLIP_MARGIN if antialias else pu.FLIP_MARGIN)
        pu.assert_pixels_close(out.image, image_ref, f"image aa={antialias}", atol=5e-5, rtol=5e-5, flips=proof)
        gi = np.random.default_rng(seed).random((8, 8, channels)).astype(np.float32)
        (out.image * dev(gi)).sum().backward()
        gg, gf, _ = orc.rasterize_backward(g2d.double(), g.feature.double(), o2p, ranges, (8, 8), image_ref,
                                           gi.astype(np.float64), orc.OracleConfig.of(cfg))
        pu.assert_grad_close(g_t.grad, gg, f"grad_gaussians2d aa={antialias}", tol=1e-3)
        pu.assert_grad_close(f_t.grad, gf, f"grad_features aa={antialias}", tol=1e-3)


@pytest.mark.parametrize("seed", range(3))
def test_visibility_and_heuristics(seed):
    """tests/test_visibility.py:34-64 (visibility == d sum(image)/d feature[:,0]) + oracle parity"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(100, 6000))
    size = (320, 200)
    g2d, depth, feat = pu.make_2d_scene(seed, n, size, scale_factor=0.2, alpha_range=(0.2, 1.0))
    cfg = RasterConfig(compute_visibility=True, compute_point_heuristic=True)
    f_t = dev(feat).requires_grad_(True)
    g_t = dev(g2d).requires_grad_(True)
    raster = gs.rasterize(g_t, dev(depth), f_t, size, cfg)
    raster.image.sum().backward()
    vis = pu.to_np(raster.visibility)
    assert vis.shape == (n,)
    assert np.allclose(pu.to_np(f_t.grad[:, 0]), vis, rtol=1e-4, atol=3e-4)
    ocfg = orc.OracleConfig.of(cfg)
    (image_ref, _, vis_ref), (o2p, ranges) = orc.rasterize(g2d, depth, feat, size, ocfg)
    pu.assert_grad_close(vis, vis_ref, "visibility")
    _, _, heur_ref = orc.rasterize_backward(g2d, feat, o2p, ranges, size, pu.to_np(raster.image),
                                            np.ones_like(image_ref), ocfg)
    pu.assert_grad_close(raster.point_heuristic, heur_ref, "point_heuristic", tol=1e-3)


def test_quantile_mode_median_depth():
    """use_alpha_blending=False + saturate_threshold=0.5 (renderer.py:203-208): forward only"""
    size = (96, 64)
    g2d, depth, _ = pu.make_2d_scene(11, 600, size, scale_factor=0.6, alpha_range=(0.3, 0.9))
    cfg = RasterConfig(use_alpha_blending=False, saturate_threshold=0.5)
    ocfg = orc.OracleConfig.of(cfg)
    o2p, ranges = orc.map_to_tiles(g2d, depth, size, ocfg)
    image_ref, alpha_ref, _ = orc.rasterize_with_tiles(g2d, depth, o2p, ranges, size, ocfg)
    out = gs.rasterize_with_tiles(dev(g2d), dev(depth), dev(o2p), dev(ranges.reshape(-1, 2)), size, cfg)
    # a flipped alpha decision moves the 0.5 crossing to another splat: the pixel then takes that splat's depth
    proof = pu.flip_proof(g2d, depth, o2p, ranges, size, ocfg)
    pu.assert_pixels_close(out.image, image_ref, "median depth", flips=proof, bound=False)
    assert (pu.to_np(out.image_weight) == alpha_ref).mean() > 0.999


def test_raster_empty():
    cfg = RasterConfig()
    ranges = torch.zeros((6, 2), dtype=torch.int32, device=DEV)
    out = gs.rasterize_with_tiles(torch.zeros((0, 7), device=DEV), torch.zeros((0, 3), device=DEV),
                                  torch.zeros((0,), dtype=torch.int32, device=DEV), ranges, (40, 30), cfg)
    assert tuple(out.image.shape) == (30, 40, 3) and float(out.image.abs().sum()) == 0.0
    assert float(out.image_weight.abs().sum()) == 0.0


# -------------------------------------------------------------------------------- projection
PROJ = [c for c in projection_cases() if c[1] == np.float32]


@pytest.mark.parametrize("name,dt,ins,exp,meta", PROJ, ids=[c[0] for c in PROJ])
def test_projection_golden(name, dt, ins, exp, meta):
    """HIP f32 vs the reference torch_lib's f64 values for the same inputs; the bar is the error of
    the reference's own f32 run against that truth (see tests/test_oracle_golden.py)."""
    truth = load_cases("projection.npz")[name[:-3] + "f64"]
    keys = ["position", "log_scaling", "rotation", "alpha_logit", "T_camera_world", "projection"]
    t = [dev(ins[k]).requires_grad_(True) for k in keys]
    points, depth, idx = hip_proj.apply(*t, meta["image_size"], meta["depth_range"], blur_cov=meta["blur_cov"])
    assert idx.dtype == torch.int64
    assert idx.shape[0] == truth["indexes"].shape[0] and (pu.to_np(idx) == truth["indexes"]).all(), "visible set"
    if idx.shape[0] == 0:
        return
    ref32 = np.abs(pu.cov_form(exp["points"]) - pu.cov_form(truth["points"])).max(0)
    ours = np.abs(pu.cov_form(points) - pu.cov_form(truth["points"])).max(0)
    scale = np.abs(pu.cov_form(truth["points"])).max(0)
    assert (ours <= 4 * ref32 + 1e-5 * scale + 1e-6).all(), f"{ours} vs reference f32 error {ref32}"
    assert np.allclose(pu.to_np(depth), truth["depth"], rtol=1e-4)
    (points.mean() + depth.mean()).backward()
    for tensor, k in zip(t, keys):
        tr = truth[f"grad_{k}"]
        s = max(float(np.abs(tr).max()), 1e-30)
        ref_err = float(np.abs(exp[f"grad_{k}"] - tr).max()) / s
        our_err = float(np.abs(pu.to_np(tensor.grad) - tr).max()) / s
        assert our_err <= 4 * ref_err + 2e-4, f"grad {k}: {our_err:.2e} vs reference f32 error {ref_err:.2e}"


@pytest.mark.parametrize("seed,n", [(0, 5000), (1, 50000), (2, 300)])
def test_projection_vs_oracle(seed, n):
    torch.manual_seed(seed)
    camera = scenes.random_camera()
    g = scenes.random_3d_gaussians(n, camera, margin=0.5, scale_factor=0.1)
    cfg = RasterConfig()
    args = [*g.shape_tensors(), camera.T_camera_world, camera.projection]
    p_ref, d_ref, i_ref = orc.project(*args, camera.image_size, camera.depth_range, blur_cov=cfg.blur_cov)
    t = [dev(a).requires_grad_(True) for a in args]
    p, d, i, ndc = hip_proj.project_with_ndc(*t, camera.image_size, camera.depth_range, cfg)
    sym = np.setxor1d(pu.to_np(i), i_ref)
    assert sym.size <= max(1, n // 20000), f"visible sets differ in {sym.size} gaussians"
    common, ia, ib = np.intersect1d(pu.to_np(i), i_ref, return_indices=True)
    assert (np.diff(pu.to_np(i)) > 0).all()
    pu.assert_grad_close(pu.cov_form(pu.to_np(p)[ia]), pu.cov_form(p_ref[ib]), "points (cov form)", tol=1e-3)
    assert np.allclose(pu.to_np(d)[ia], d_ref[ib], rtol=1e-5)
    # ndc depth: bit-exact function of the depth the kernel itself produced
    assert (pu.to_np(ndc) == orc.ndc_depth(pu.to_np(d), camera.near_plane, camera.far_plane)).all()
    if sym.size == 0:
        gen = torch.Generator().manual_seed(seed)
        gp, gd = torch.rand(p.shape, generator=gen), torch.rand(d.shape, generator=gen)
        ((p * dev(gp)).sum() + (d * dev(gd)).sum()).backward()
        # f32 gradients of these far-away random cameras are ill-conditioned (the reference's own f32
        # run is ~1e-3 off its f64 run): measure both f32 implementations against the oracle in f64
        args64 = [a.double() for a in args]
        truth = orc.project_backward(*args64, camera.image_size, i_ref, gp.double().numpy(), gd.double().numpy(),
                                     blur_cov=cfg.blur_cov)
        cpu32 = orc.project_backward(*args, camera.image_size, i_ref, gp.numpy(), gd.numpy(), blur_cov=cfg.blur_cov)
        for tensor, tr, c32, k in zip(t, truth, cpu32, ["position", "log_scaling", "rotation", "alpha_logit", "T", "proj"]):
            s = max(float(np.abs(tr).max()), 1e-30)
            cpu_err = float(np.abs(c32 - tr).max()) / s
            hip_err = float(np.abs(pu.to_np(tensor.grad) - tr).max()) / s
            assert hip_err <= 4 * cpu_err + 2e-4, f"d_{k}: HIP f32 error {hip_err:.2e} vs CPU f32 error {cpu_err:.2e}"


# ---------------------------------------------------------------------------------------- SH
SHC = [c for c in sh_cases() if c[1] == np.float32]


@pytest.mark.parametrize("name,dt,ins,indexes,exp", SHC, ids=[c[0] for c in SHC])
def test_sh_golden(name, dt, ins, indexes, exp):
    """reference bar: atol 1e-5 (tests/util.py:62-63) on outputs and gradients"""
    params, points, cam = (dev(ins[k]).requires_grad_(True) for k in ("params", "points", "camera_pos"))
    out = gs.evaluate_sh_at(params, points, dev(indexes), cam)
    assert np.allclose(pu.to_np(out), exp["out"], atol=1e-5)
    out.mean().backward()
    assert np.allclose(pu.to_np(params.grad), exp["grad_params"], atol=1e-5)
    assert np.allclose(pu.to_np(points.grad), exp["grad_points"], atol=1e-5, rtol=1e-4)
    assert np.allclose(pu.to_np(cam.grad), exp["grad_camera_pos"], atol=1e-5, rtol=1e-4)


# -------------------------------------------------------------------------- render_gaussians
E2E_CASES = [(0, 2000, (160, 120), 3, False), (1, 20000, (320, 240), 3, True), (2, 5000, (200, 200), 0, False),
             (3, 3000, (129, 65), 2, True)]


@pytest.mark.parametrize("seed,n,size,deg,depth_mode", E2E_CASES)
def test_render_gaussians_stagewise(seed, n, size, deg, depth_mode, frame_path):
    """render_gaussians == the composition of the HIP operators, and every stage of that composition
    matches the oracle when the oracle is fed the HIP stage's own inputs (tight tolerances: no
    compounding of f32 rounding through the pipeline)."""
    _render_gaussians_stagewise(seed, n, size, deg, depth_mode, RasterConfig())


@pytest.mark.parametrize("depth_mode", [False, True])
@pytest.mark.parametrize("fid", list(cc.FRAMES))
def test_render_gaussians_stagewise_at_other_settings(fid, depth_mode, frame_path):
    """the same at tile sizes 8 and 32 and with every threshold, clamp, margin and blur away from its default"""
    s = cc.FRAME_SCENE
    _render_gaussians_stagewise(s["seed"], s["n"], s["size"], s["sh_degree"], depth_mode, cc.frame_config(fid))


def _render_gaussians_stagewise(seed, n, size, deg, depth_mode, cfg):
    g, camera = scenes.benchmark_scene(n, size, sh_degree=deg, seed=seed)
    ocfg = orc.OracleConfig.of(cfg)
    gen = torch.Generator().manual_seed(seed + 7)
    gi = torch.rand(size[1], size[0], 3, generator=gen)
    gdm, gvm = torch.rand(size[1], size[0], generator=gen), torch.rand(size[1], size[0], generator=gen) * 0.1
    gd = g.to(DEV).requires_grad_(True)
    cam = camera.to(device=DEV)

    # --- the composition, holding on to the intermediates
    g2d, depths, idx, ndc = hip_proj.project_with_ndc(*gd.shape_tensors(), cam.T_camera_world, cam.projection,
                                                      cam.image_size, cam.depth_range, cfg)
    feats = gs.evaluate_sh_at(gd.feature, gd.position.detach(), idx, cam.camera_position)
    g2d.retain_grad(); depths.retain_grad(); feats.retain_grad()
    from taichi_gaussian_rasterizer_amd.renderer import render_projected
    r = render_projected(idx, g2d, feats, depths, cam, cfg, render_depth=depth_mode, ndc_depths=ndc)
    loss = (r.image * dev(gi)).sum()
    if depth_mode:
        loss = loss + (r.depth * dev(gdm)).sum() + (r.depth_var * dev(gvm)).sum()
    loss.backward()

    # --- render_gaussians is exactly this composition
    r2 = gs.render_gaussians(g.to(DEV), cam, cfg, use_sh=True, render_depth=depth_mode)
    assert torch.equal(r2.image, r.image) and torch.equal(r2.points_in_view, idx)
    assert torch.equal(r2.gaussians2d, g2d.detach())

    # --- stage: SH, given the HIP index list
    cam_pos = pu.to_np(cam.camera_position)
    f_ref = orc.evaluate_sh_at(g.feature.numpy(), g.position.numpy(), pu.to_np(idx), cam_pos)
    assert np.allclose(pu.to_np(feats), f_ref, atol=1e-5)

    # --- stage: mapper, given HIP points + ndc depth: bit-exact
    p_np, d_np, ndc_np = pu.to_np(g2d), pu.to_np(depths), pu.to_np(ndc)
    assert (ndc_np == orc.ndc_depth(d_np, camera.near_plane, camera.far_plane)).all()
    o2p_ref, ranges_ref = orc.map_to_tiles(p_np, ndc_np, size, ocfg)
    o2p, ranges = gs.map_to_tiles(g2d.detach(), ndc, size, cfg)
    assert (pu.to_np(o2p) == o2p_ref).all() and (pu.to_np(ranges) == ranges_ref).all()

    # --- stage: rasterizer forward/backward, given HIP points/features
    f_np = pu.to_np(feats)
    feats_r = np.concatenate([d_np, d_np ** 2, f_np], 1).astype(np.float32) if depth_mode else f_np
    image_ref, alpha_ref, _ = orc.rasterize_with_tiles(p_np, feats_r, o2p_ref, ranges_ref, size, ocfg)
    proof = pu.flip_proof(p_np, feats_r, o2p_ref, ranges_ref, size, ocfg, bar=cc.raster_bar(cfg, p_np))
    g_img = np.zeros_like(image_ref)
    if depth_mode:
        pu.assert_pixels_close(r.image, image_ref[..., 2:], "image", flips=proof.channels(slice(2, None)))
        w = alpha_ref + np.float32(1e-6)
        d_img = image_ref[..., 0] / w
        pu.assert_pixels_close(r.depth, d_img, "depth", atol=1e-4, rtol=1e-4, flips=proof.weight(), bound=False)
        pu.assert_pixels_close(r.depth_var, image_ref[..., 1] / w - d_img ** 2, "depth_var", atol=2e-3, rtol=1e-3,
                               flips=proof.weight(), bound=False)
        hip_img = np.concatenate([pu.to_np(r.depth * (r.image_weight + 1e-6))[..., None],
                                  pu.to_np((r.depth_var + r.depth ** 2) * (r.image_weight + 1e-6))[..., None],
                                  pu.to_np(r.image)], -1)
        w_h = pu.to_np(r.image_weight) + np.float32(1e-6)
        d_h = pu.to_np(r.depth)
        g_img[..., 2:] = gi.numpy()
        g_img[..., 0] = (gdm.numpy() - 2 * d_h * gvm.numpy()) / w_h
        g_img[..., 1] = gvm.numpy() / w_h
    else:
        pu.assert_pixels_close(r.image, image_ref, "image", flips=proof)
        hip_img = pu.to_np(r.image)
        g_img[...] = gi.numpy()
    pu.assert_pixels_close(r.image_weight, alpha_ref, "image_weight", flips=proof.weight())
    gg, gf, heur = orc.rasterize_backward(p_np, feats_r, o2p_ref, ranges_ref, size, hip_img.astype(np.float32), g_img,
                                          ocfg)
    if cfg.compute_point_heuristic:
        pu.assert_grad_close(r.point_heuristic, heur, "point_heuristic", tol=1e-3)
    gdepth_ref = np.zeros_like(d_np)
    if depth_mode:
        gdepth_ref = gf[:, 0:1] + 2 * d_np * gf[:, 1:2]
        gf = gf[:, 2:]
        pu.assert_grad_close(depths.grad, gdepth_ref, "d depth", tol=1e-3)
    pu.assert_grad_close(g2d.grad, gg, "d gaussians2d", tol=1e-3)
    pu.assert_grad_close(feats.grad, gf, "d features", tol=1e-3)

    # --- stage: projection / SH backward, given the HIP upstream gradients
    args = [*g.shape_tensors(), camera.T_camera_world, camera.projection]
    up_d = pu.to_np(depths.grad) if depths.grad is not None else np.zeros_like(d_np)
    args64 = [a.double() for a in args]
    truth = orc.project_backward(*args64, size, pu.to_np(idx), pu.to_np(g2d.grad).astype(np.float64),
                                 up_d.astype(np.float64), blur_cov=cfg.blur_cov, clamp_margin=cfg.clamp_margin)
    cpu32 = orc.project_backward(*args, size, pu.to_np(idx), pu.to_np(g2d.grad), up_d, blur_cov=cfg.blur_cov,
                                 clamp_margin=cfg.clamp_margin)
    for name, tr, c32 in zip(("position", "log_scaling", "rotation", "alpha_logit"), truth, cpu32):
        sc = max(float(np.abs(tr).max()), 1e-30)
        cpu_err = float(np.abs(c32 - tr).max()) / sc
        hip_err = float(np.abs(pu.to_np(getattr(gd, name).grad) - tr).max()) / sc
        assert hip_err <= 4 * cpu_err + 2e-4, f"d_{name}: HIP f32 error {hip_err:.2e} vs CPU f32 error {cpu_err:.2e}"
    dfeat_ref, _, _ = orc.evaluate_sh_at_backward(g.feature.numpy(), g.position.numpy(), pu.to_np(idx), cam_pos,
                                                  pu.to_np(feats.grad))
    assert np.allclose(pu.to_np(gd.feature.grad), dfeat_ref, atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize("seed,n,size,deg,depth_mode", E2E_CASES)
def test_render_gaussians_end_to_end_vs_oracle(seed, n, size, deg, depth_mode):
    """whole pipeline on the GPU vs whole pipeline on the CPU oracle.  f32 rounding of the projected
    means (1e-7 * ~1e3 px) is amplified by the blend, so the end-to-end bar is looser than the
    per-stage one (see the stagewise test for the tight comparison)."""
    g, camera = scenes.benchmark_scene(n, size, sh_degree=deg, seed=seed)
    cfg = RasterConfig()
    gi = torch.rand(size[1], size[0], 3, generator=torch.Generator().manual_seed(seed + 7))
    ref = pu.oracle_render(g, camera, cfg, use_sh=True, render_depth=depth_mode, grads=dict(image=gi.numpy()))
    ref64 = pu.oracle_render(g, camera, cfg, use_sh=True, render_depth=depth_mode,
                             grads=dict(image=gi.numpy().astype(np.float64)), dtype=np.float64)
    gd = g.to(DEV).requires_grad_(True)
    r = gs.render_gaussians(gd, camera.to(device=DEV), cfg, use_sh=True, render_depth=depth_mode)
    assert (pu.to_np(r.points_in_view) == ref["indexes"]).all()
    pu.assert_pixels_close(r.image, ref["image"], "image", atol=1e-3, rtol=1e-3, flips=ref["flips"])
    pu.assert_pixels_close(r.image_weight, ref["alpha"], "image_weight", atol=1e-3, rtol=1e-3,
                           flips=ref["flips"].weight())
    (r.image * dev(gi)).sum().backward()
    relgap = np.full(n, np.inf)
    relgap[ref["indexes"]] = pu.relative_eigen_gap(ref["points"])
    for name, key in (("position", "d_position"), ("log_scaling", "d_log_scaling"), ("rotation", "d_rotation"),
                      ("alpha_logit", "d_alpha_logit"), ("feature", "d_feature")):
        rep = pu.assert_rows_close_e2e(getattr(gd, name).grad, ref[key], ref64[key], relgap, f"grad {name}")
        print(f"e2e seed {seed} {name}: {rep}")


# ------------------------------------------------------------------- config 1 on the GPU path
def test_config1_fit_loop_gpu():
    """BASELINE config 1 caller shape (examples/fit_image_gaussians.py:101-123) through the HIP
    operators; first-step loss equals the CPU oracle's for the same seed."""
    import oracle_ops
    from test_config1_fit_cpu import fit_loop
    losses_gpu, raster = fit_loop(gs.rasterize, DEV, steps=8)
    losses_cpu, _ = fit_loop(oracle_ops.rasterize, "cpu", steps=2)
    assert abs(losses_gpu[0] - losses_cpu[0]) <= 1e-5 * abs(losses_cpu[0])
    assert abs(losses_gpu[1] - losses_cpu[1]) <= 1e-3 * abs(losses_cpu[1])
    assert all(b < a for a, b in zip(losses_gpu, losses_gpu[1:]))
    assert raster.visibility.shape == (2000,) and raster.point_heuristic.shape == (2000, 2)


# ------------------------------------------------------------- tile-strip sharding on one GPU
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_strips_on_one_gpu(world):
    """the per-rank work of parallel.render_gaussians_sharded, ranks emulated one after another on a
    single GPU: strips tile the full image, summed partial gradients equal the full gradients"""
    _sharded_strips_on_one_gpu(world, RasterConfig())


def test_sharded_strips_on_one_gpu_at_other_settings():
    """tile size 32 (strips of 32 rows; 176 is no multiple) and frame_b's thresholds, clamp, margin and blur"""
    _sharded_strips_on_one_gpu(2, cc.frame_config("frame_b"))


def _sharded_strips_on_one_gpu(world, cfg):
    from taichi_gaussian_rasterizer_amd import parallel
    size, n = (200, 176), 6000
    g, camera = scenes.benchmark_scene(n, size, sh_degree=3, seed=4)
    cam = camera.to(device=DEV)
    gi = dev(torch.rand(size[1], size[0], 3, generator=torch.Generator().manual_seed(9)))
    full = g.to(DEV).requires_grad_(True)
    r = gs.render_gaussians(full, cam, cfg, use_sh=True)
    (r.image * gi).sum().backward()
    strips, sums = [], None
    for rank in range(world):
        gr = g.to(DEV).requires_grad_(True)
        rr = parallel.render_gaussians_sharded(gr, cam, cfg, use_sh=True, rank=rank, world_size=world)
        y0, y1 = rr.strip
        assert rr.bands == [(y0, y1)] and torch.equal(rr.gaussians2d, r.gaussians2d)
        (rr.image * gi[y0:y1]).sum().backward()
        strips.append(rr.image.detach())
        grads = {k: v.grad.clone() for k, v in gr.items()}
        sums = grads if sums is None else {k: sums[k] + grads[k] for k in sums}
    # without a process group the all-reduce is the identity, so the per-rank gradients are the
    # partial sums of the replicated backward; projection/SH backward are linear in the upstream grads
    assert torch.equal(torch.cat(strips, 0), r.image.detach())
    for k, v in full.items():
        pu.assert_grad_close(sums[k], v.grad, f"summed partial grad {k}", tol=1e-4)
    # the same with the composed operators (the path taken when the fused frame does not apply)
    strips2 = []
    for rank in range(world):
        rr = parallel.render_gaussians_sharded(g.to(DEV), cam, cfg, use_sh=True, rank=rank, world_size=world,
                                               ops=parallel.default_ops())
        strips2.append(rr.image.detach())
    # band by band on shifted means: a marginal tile decision can differ from the full frame's (the mapper rounds
    # loy = my - ey once more), which moves the 64-splat group boundaries at which the forward may stop a saturated
    # region -- below forward_cut * |feature| = 1e-6 per pixel, but no longer bit for bit (the kernel-level shards
    # above are: they work in full-image coordinates)
    assert torch.allclose(torch.cat(strips2, 0), r.image.detach(), rtol=0, atol=2e-6)


@pytest.mark.parametrize("interleave", [0, 1])
def test_rank_local_sh_covers_every_listed_splat(interleave):
    _rank_local_sh_covers_every_listed_splat(interleave, RasterConfig())


@pytest.mark.parametrize("interleave", [0, 1])
@pytest.mark.parametrize("thr", [1e-4, 0.3], ids=["thr_small", "thr_big"])
def test_rank_local_sh_covers_every_listed_splat_at_other_thresholds(thr, interleave):
    """the reach test of gs_sh_fwd_shard has its own copy of the threshold (sh.hip: touch.thr): at 1e-4 the mapper
    lists splats 1.3x further out than at 1/255, at 0.3 a default extent would still cover them"""
    _rank_local_sh_covers_every_listed_splat(interleave, RasterConfig(alpha_threshold=thr))


def _rank_local_sh_covers_every_listed_splat(interleave, cfg):
    """gs_sh_fwd_shard evaluates colours only for the splats that can reach a rank's rows (0.5 elsewhere): its row test
    must be a superset of the mapper's tile lists.  Long, thin, rotated splats over one-tile-row strips (16 ranks on a
    256-px image, also dealt row by row) are the hard case -- the reference's tile test accepts tiles just outside a
    splat's bounding box; every strip must still equal the rows of the unsharded image bit for bit."""
    from taichi_gaussian_rasterizer_amd import parallel
    size, n, world = (320, 256), 4000, 16
    g, camera = scenes.benchmark_scene(n, size, sh_degree=3, seed=11)
    gen = torch.Generator().manual_seed(12)
    g.log_scaling[:, 0] += 1.5 + torch.rand(n, generator=gen)     # 4.5 - 12 x longer along one axis
    g.log_scaling[:, 1:] -= 0.7
    cam = camera.to(device=DEV)
    full = gs.render_gaussians(g.to(DEV), cam, cfg, use_sh=True)
    rows = []
    for rank in range(world):
        rr = parallel.render_gaussians_sharded(g.to(DEV), cam, cfg, use_sh=True, rank=rank, world_size=world,
                                               interleave=interleave)
        assert torch.equal(rr.image, full.image[parallel.owned_pixel_rows(rr.bands).to(DEV)]), rank
        rows.append(rr.image.shape[0])
    assert sum(rows) == size[1]


# ------------------------------------------- full-size properties (BASELINE config 3 shapes)
def test_full_size_c3_properties():
    """1M Gaussians at 2048x2048, too large for the CPU oracle in a unit test: size-independent
    properties instead -- sortedness and partition of the mapper output, the visibility identity
    (tests/test_visibility.py), linearity of the backward in the upstream gradient, determinism of
    the forward."""
    n, size = 1_000_000, (2048, 2048)
    g, camera = scenes.benchmark_scene(n, size, sh_degree=3, seed=0)
    cam = camera.to(device=DEV)
    # saturate_threshold = 1: the backward never stops a pixel early, so the visibility identity is
    # exact up to rounding (at 0.9999 the forward keeps blending a tail the backward drops)
    cfg = RasterConfig(compute_visibility=True, saturate_threshold=1.0)
    gd = g.to(DEV)
    p2d, depth, idx, ndc = hip_proj.project_with_ndc(*gd.shape_tensors(), cam.T_camera_world, cam.projection,
                                                     cam.image_size, cam.depth_range, cfg)
    V = p2d.shape[0]
    assert 0.7 * n < V <= n and bool((idx[1:] > idx[:-1]).all())
    o2p, ranges, keys = gs.map_to_tiles(p2d, ndc, size, cfg, return_keys=True)
    K = o2p.shape[0]
    assert keys.dtype == torch.int64 and bool((keys[1:] >= keys[:-1]).all()), "keys not sorted"
    same = keys[1:] == keys[:-1]
    assert bool((o2p[1:][same] > o2p[:-1][same]).all()), "ties not in ascending gaussian order"
    r = ranges.view(-1, 2).long()
    nonempty = r[:, 1] > r[:, 0]
    starts, ends = r[nonempty, 0], r[nonempty, 1]
    assert int(starts[0]) == 0 and int(ends[-1]) == K and bool((starts[1:] == ends[:-1]).all())
    assert int(r[~nonempty].abs().sum()) == 0
    tile_of = (keys >> 32)
    assert bool((tile_of[starts] == torch.nonzero(nonempty).squeeze(1)).all())
    # checksum of checksums: every visible gaussian's overlap count equals the reference-shaped count
    counts = torch.zeros(V, dtype=torch.int64, device=DEV).index_add_(0, o2p.long(), torch.ones(K, dtype=torch.int64, device=DEV))
    o2p_b, ranges_b = map_to_tiles_reference_stages(p2d, ndc, size, cfg)
    assert torch.equal(o2p_b, o2p) and torch.equal(ranges_b, ranges)
    assert int(counts.sum()) == K

    feats = gs.evaluate_sh_at(gd.feature, gd.position, idx, cam.camera_position).requires_grad_(True)
    p_t = p2d.detach().requires_grad_(True)
    out = gs.rasterize_with_tiles(p_t, feats, o2p, ranges.view(-1, 2), size, cfg)
    out2 = gs.rasterize_with_tiles(p2d.detach(), feats.detach(), o2p, ranges.view(-1, 2), size, cfg)
    assert torch.equal(out.image, out2.image), "forward is not deterministic"
    assert float(out.image_weight.max()) <= 1.0 + 1e-5 and float(out.image_weight.min()) >= 0.0
    out.image.sum().backward()
    vis = out.visibility
    assert torch.allclose(feats.grad[:, 0], vis, rtol=1e-3, atol=1e-3)
    g1 = p_t.grad.clone()
    p_t.grad = None
    feats.grad = None
    out = gs.rasterize_with_tiles(p_t, feats, o2p, ranges.view(-1, 2), size, cfg)
    (out.image.sum() * 2.0).backward()
    pu.assert_grad_close(p_t.grad, 2.0 * g1, "backward linearity", tol=1e-4)


# ------------------------------------------------------------------------------ fused frame
@pytest.mark.parametrize("depth_mode,heur", [(False, False), (True, False), (False, True)])
def test_fused_frame_equals_composed_operators(depth_mode, heur, frame_path):
    """fused.py (one autograd node, device-side counts) against the operator-by-operator composition:
    identical forward, gradients equal up to the order of the float atomics; repeated frames exercise
    the capacity hint and the overflow re-run."""
    from taichi_gaussian_rasterizer_amd import fused
    from taichi_gaussian_rasterizer_amd.renderer import render_projected
    size = (256, 192)
    cfg = RasterConfig(compute_visibility=heur, compute_point_heuristic=heur)
    gi = dev(torch.rand(size[1], size[0], 3, generator=torch.Generator().manual_seed(3)))
    fused._K_HINT.clear()
    for it, n in enumerate((8000, 8000, 30000, 500)):  # 3rd frame overflows the hint of the 2nd (same key? no: n differs)
        g, camera = scenes.benchmark_scene(n, size, sh_degree=3, seed=it)
        cam = camera.to(device=DEV)
        a = g.to(DEV).requires_grad_(True)
        r = gs.render_gaussians(a, cam, cfg, use_sh=True, render_depth=depth_mode)
        b = g.to(DEV).requires_grad_(True)
        g2d, depths, idx, ndc = hip_proj.project_with_ndc(*b.shape_tensors(), cam.T_camera_world, cam.projection,
                                                          cam.image_size, cam.depth_range, cfg)
        feats = gs.evaluate_sh_at(b.feature, b.position.detach(), idx, cam.camera_position)
        r2 = render_projected(idx, g2d, feats, depths, cam, cfg, render_depth=depth_mode, ndc_depths=ndc)
        assert torch.equal(r.points_in_view, r2.points_in_view) and torch.equal(r.gaussians2d, r2.gaussians2d)
        assert torch.equal(r.image, r2.image) and torch.equal(r.image_weight, r2.image_weight)
        la, lb = (r.image * gi).sum(), (r2.image * gi).sum()
        if depth_mode:
            assert torch.equal(r.depth, r2.depth)
            la, lb = la + r.depth.sum() + 0.1 * r.depth_var.sum(), lb + r2.depth.sum() + 0.1 * r2.depth_var.sum()
        la.backward()
        lb.backward()
        # same kernels, different order of the float atomics; the projection adjoint amplifies that noise for
        # near-isotropic splats (1 / eigenvalue gap), so the bound is loose -- a wiring error would be O(1)
        for k, t in a.items():
            pu.assert_grad_close(t.grad, getattr(b, k).grad, f"fused grad {k}", tol=1e-3)
        if heur:
            pu.assert_grad_close(r.point_visibility, r2.point_visibility, "visibility", tol=1e-5)
            pu.assert_grad_close(r.point_heuristic, r2.point_heuristic, "heuristic", tol=1e-4)


@pytest.mark.parametrize("n", [1, 63, 1023, 1024, 1025, 2049, 3072])
def test_fused_frame_at_binning_workgroup_edges(n, frame_path):
    """the frame calls fold the mapper's region binning into the projection's compaction pass, 1024 staged rows per
    workgroup (mapper.hip: compact_bin_kernel); counts at and around multiples of that must give the composed operators'
    frame bit for bit"""
    from taichi_gaussian_rasterizer_amd.renderer import render_projected
    size = (160, 96)
    cfg = RasterConfig()
    g, camera = scenes.benchmark_scene(n, size, sh_degree=1, seed=100 + n)
    cam = camera.to(device=DEV)
    a = g.to(DEV).requires_grad_(True)
    r = gs.render_gaussians(a, cam, cfg, use_sh=True)
    b = g.to(DEV).requires_grad_(True)
    g2d, depths, idx, ndc = hip_proj.project_with_ndc(*b.shape_tensors(), cam.T_camera_world, cam.projection,
                                                      cam.image_size, cam.depth_range, cfg)
    feats = gs.evaluate_sh_at(b.feature, b.position.detach(), idx, cam.camera_position)
    r2 = render_projected(idx, g2d, feats, depths, cam, cfg, ndc_depths=ndc)
    assert torch.equal(r.points_in_view, r2.points_in_view) and torch.equal(r.gaussians2d, r2.gaussians2d)
    assert torch.equal(r.image, r2.image) and torch.equal(r.image_weight, r2.image_weight)
    r.image.sum().backward()
    r2.image.sum().backward()
    for k, t in a.items():
        pu.assert_grad_close(t.grad, getattr(b, k).grad, f"grad {k}", tol=1e-3)


@pytest.mark.parametrize("depth_mode", [False, True])
def test_fused_frame_gradients_through_projected_splats(depth_mode, frame_path):
    """a loss that also reads `gaussians2d` and `point_depth` (a regulariser on the projected splats): the fused
    node adds those upstream gradients to the rasterizer's rows; unused outputs get no materialized zeros"""
    from taichi_gaussian_rasterizer_amd.renderer import render_projected
    size, n = (192, 128), 5000
    cfg = RasterConfig()
    g, camera = scenes.benchmark_scene(n, size, sh_degree=2, seed=11)
    cam = camera.to(device=DEV)
    gen = torch.Generator().manual_seed(5)
    gi = dev(torch.rand(size[1], size[0], 3, generator=gen))
    grads = []
    for fused_path in (True, False):
        a = g.to(DEV).requires_grad_(True)
        if fused_path:
            r = gs.render_gaussians(a, cam, cfg, use_sh=True, render_depth=depth_mode)
        else:
            g2d, depths, idx, ndc = hip_proj.project_with_ndc(*a.shape_tensors(), cam.T_camera_world, cam.projection,
                                                              cam.image_size, cam.depth_range, cfg)
            feats = gs.evaluate_sh_at(a.feature, a.position.detach(), idx, cam.camera_position)
            r = render_projected(idx, g2d, feats, depths, cam, cfg, render_depth=depth_mode, ndc_depths=ndc)
        V = r.gaussians2d.shape[0]
        w2d = dev(torch.rand(V, 7, generator=torch.Generator().manual_seed(6)))
        wd = dev(torch.rand(V, generator=torch.Generator().manual_seed(7)))
        loss = (r.image * gi).sum() + 0.01 * (r.gaussians2d * w2d).sum() + 0.1 * (r.point_depth.reshape(-1) * wd).sum()
        loss.backward()
        grads.append({k: t.grad.clone() for k, t in a.items()})
    for k in grads[0]:
        pu.assert_grad_close(grads[0][k], grads[1][k], f"fused grad {k} with splat/depth terms", tol=1e-4)
    # only the splats are used: no image gradient at all
    a = g.to(DEV).requires_grad_(True)
    r = gs.render_gaussians(a, cam, cfg, use_sh=True, render_depth=depth_mode)
    r.gaussians2d.sum().backward()
    assert a.position.grad is not None and torch.isfinite(a.position.grad).all()
    assert a.feature.grad is None or float(a.feature.grad.abs().max()) == 0.0


@pytest.mark.parametrize("channels,depth_mode", [(3, False), (6, True), (1, False)])
def test_fused_frame_plain_features_and_camera_gradients(channels, depth_mode, frame_path):
    """render_gaussians(use_sh=False) -- the reference's default -- through the fused node: plain (N, C) features are
    gathered by gs_feature_gather_fwd, and with no SH in the way the camera matrices may require gradients too"""
    from taichi_gaussian_rasterizer_amd.renderer import render_projected
    size, n = (224, 160), 6000
    cfg = RasterConfig()
    g, camera = scenes.benchmark_scene(n, size, sh_degree=0, seed=13)
    feats = torch.rand(n, channels, generator=torch.Generator().manual_seed(8))
    g = g.replace(feature=feats)
    gi = dev(torch.rand(size[1], size[0], channels, generator=torch.Generator().manual_seed(3)))
    grads = []
    for fused_path in (True, False):
        cam = camera.to(device=DEV)
        cam.T_camera_world.requires_grad_(True)
        cam.projection.requires_grad_(True)
        a = g.to(DEV).requires_grad_(True)
        if fused_path:
            r = gs.render_gaussians(a, cam, cfg, use_sh=False, render_depth=depth_mode)
        else:
            g2d, depths, idx, ndc = hip_proj.project_with_ndc(*a.shape_tensors(), cam.T_camera_world, cam.projection,
                                                              cam.image_size, cam.depth_range, cfg)
            r = render_projected(idx, g2d, a.feature[idx], depths, cam, cfg, render_depth=depth_mode, ndc_depths=ndc)
        loss = (r.image * gi).sum()
        if depth_mode:
            loss = loss + r.depth.sum()
        loss.backward()
        grads.append((r.image.detach().clone(), {k: t.grad.clone() for k, t in a.items()},
                      cam.T_camera_world.grad.clone(), cam.projection.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0])
    for k in grads[0][1]:
        pu.assert_grad_close(grads[0][1][k], grads[1][1][k], f"plain-feature grad {k}", tol=1e-3)
    pu.assert_grad_close(grads[0][2], grads[1][2], "grad T_camera_world", tol=1e-3)
    pu.assert_grad_close(grads[0][3], grads[1][3], "grad projection", tol=1e-3)


def test_fused_frame_sh_with_camera_gradients(frame_path):
    """pose refinement: T_camera_world requires grad while the colours are SH -- the view direction depends on the camera
    centre inverse(T)[:3, 3] (reference perspective/params.py:76-78).  Fused node (SH adjoint returns dL/d centre, the
    4x4 inverse is differentiated by hand) against the composed operators, where torch differentiates the inverse"""
    from taichi_gaussian_rasterizer_amd.renderer import render_projected
    size, n = (200, 144), 5000
    cfg = RasterConfig()
    g, camera = scenes.benchmark_scene(n, size, sh_degree=3, seed=17)
    g = g.replace(feature=g.feature + 0.3 * torch.randn(g.feature.shape, generator=torch.Generator().manual_seed(2)))
    gi = dev(torch.rand(size[1], size[0], 3, generator=torch.Generator().manual_seed(3)))
    tilt = torch.eye(4)
    tilt[:3, :3] = torch.linalg.qr(torch.eye(3) + 0.05 * torch.randn(3, 3, generator=torch.Generator().manual_seed(4))).Q
    tilt[:3, 3] = torch.tensor([0.02, -0.01, 0.03])
    out = []
    for fused_path in (True, False):
        cam = camera.transformed(tilt).to(device=DEV)
        cam.T_camera_world.requires_grad_(True)
        cam.projection.requires_grad_(True)
        a = g.to(DEV).requires_grad_(True)
        if fused_path:
            r = gs.render_gaussians(a, cam, cfg, use_sh=True)
        else:
            g2d, depths, idx, ndc = hip_proj.project_with_ndc(*a.shape_tensors(), cam.T_camera_world, cam.projection,
                                                              cam.image_size, cam.depth_range, cfg)
            colours = gs.evaluate_sh_at(a.feature, a.position.detach(), idx, cam.camera_position)
            r = render_projected(idx, g2d, colours, depths, cam, cfg, ndc_depths=ndc)
        (r.image * gi).sum().backward()
        out.append((r.image.detach().clone(), cam.T_camera_world.grad.clone(), cam.projection.grad.clone(),
                    a.feature.grad.clone()))
    assert torch.allclose(out[0][0], out[1][0], rtol=0, atol=2e-6)   # camera centre: device kernel vs torch inverse
    pu.assert_grad_close(out[0][1], out[1][1], "grad T_camera_world (projection + SH view direction)", tol=2e-3)
    pu.assert_grad_close(out[0][2], out[1][2], "grad projection", tol=1e-3)
    pu.assert_grad_close(out[0][3], out[1][3], "grad feature", tol=1e-3)


@pytest.mark.parametrize("nb", ["2", "4"])
def test_fused_frame_splits_heavy_tiles(nb, monkeypatch, frame_path):
    _fused_frame_splits_heavy_tiles(nb, monkeypatch, RasterConfig())


def test_fused_frame_splits_heavy_tiles_at_other_settings(monkeypatch, frame_path):
    """the 8x8 workgroups of a split tile with a low threshold, a clamp of 0.6 and a saturation level of 0.95"""
    _fused_frame_splits_heavy_tiles("2", monkeypatch, RasterConfig(**cc.CONFIGS["mixed"]))


def _fused_frame_splits_heavy_tiles(nb, monkeypatch, cfg):
    """the mapper marks the fullest tiles of its launch order (counts_out[3]) and the rasterizer gives each of them
    four 8x8 workgroups; with 16x16 / 16x8 wave regions forced on a small, crowded frame a quarter of the tiles take
    that path: pixels must be identical to the unsplit rasterizer, gradients equal up to summation order"""
    from taichi_gaussian_rasterizer_amd.renderer import render_projected
    size, n = (256, 192), 12000
    g, camera = scenes.benchmark_scene(n, size, sh_degree=1, seed=21)
    cam = camera.to(device=DEV)
    gi = dev(torch.rand(size[1], size[0], 3, generator=torch.Generator().manual_seed(3)))
    b = g.to(DEV).requires_grad_(True)            # composed operators: no launch order, nothing is split
    g2d, depths, idx, ndc = hip_proj.project_with_ndc(*b.shape_tensors(), cam.T_camera_world, cam.projection,
                                                      cam.image_size, cam.depth_range, cfg)
    feats = gs.evaluate_sh_at(b.feature, b.position.detach(), idx, cam.camera_position)
    r2 = render_projected(idx, g2d, feats, depths, cam, cfg, render_depth=False, ndc_depths=ndc)
    (r2.image * gi).sum().backward()
    from taichi_gaussian_rasterizer_amd import _native as nv
    monkeypatch.setitem(nv.TUNING, "wave_sub_blocks", int(nb))
    a = g.to(DEV).requires_grad_(True)
    r = gs.render_gaussians(a, cam, cfg, use_sh=True)
    (r.image * gi).sum().backward()
    # same per-pixel arithmetic; only the saturation cut (all pixels of a wave's region below 2^-20 transmittance)
    # can fall at a different splat for an 8x8 quadrant than for the whole region: < 1e-6 per pixel
    assert torch.allclose(r.image, r2.image, rtol=0, atol=2e-6)
    assert torch.allclose(r.image_weight, r2.image_weight, rtol=0, atol=2e-6)
    for k, t in a.items():
        pu.assert_grad_close(t.grad, getattr(b, k).grad, f"grad {k} with split tiles", tol=1e-3)


@pytest.mark.parametrize("n,first_frame", [(8000, False), (30000, True)], ids=["poisoned_hint", "first_frame"])
def test_fused_frame_capacity_overflow_rerun(n, first_frame):
    """first_frame: a shape without a hint starts at the smallest capacity class (65 536 overlaps); this scene has more,
    so its first frame is the re-run after an overflow, and it must give the bits of a later frame with a warm hint"""
    from taichi_gaussian_rasterizer_amd import fused
    size = (256, 192)
    cfg = RasterConfig()
    g, camera = scenes.benchmark_scene(n, size, sh_degree=1, seed=0)
    cam = camera.to(device=DEV)
    if first_frame:
        fused._K_HINT.clear()
    ref = gs.render_gaussians(g.to(DEV), cam, cfg, use_sh=True)
    key = next(iter(k for k in fused._K_HINT if k[0] == n and k[1] == size[0]))
    true_k, true_max = fused._K_HINT[key]
    if first_frame:
        assert true_k > 65536
    else:
        fused._K_HINT[key] = (true_k // 3, 8)  # poison the hints: the frame must detect the overflow and re-run,
    again = gs.render_gaussians(g.to(DEV), cam, cfg, use_sh=True)  # and the catch-all sort must cover fuller tiles
    assert torch.equal(again.image, ref.image) and fused._K_HINT[key][0] == true_k


# ----------------------------------------------- remaining render_gaussians options (a15)
def test_render_gaussians_plain_features_median_depth_depth16_antialias(frame_path):
    """use_sh=False (feature gather), render_median_depth (second, non-blending raster pass,
    renderer.py:203-208), use_depth16 keys (tile_mapper.py:47-64) and the antialiased pdf through
    render_gaussians (the fused frame covers all of them), against the oracle fed the same projected splats."""
    size, n = (160, 112), 4000
    torch.manual_seed(5)
    camera = scenes.benchmark_camera(size)
    g = scenes.random_3d_gaussians(n, camera, scale_factor=1.5, margin=0.1)
    cam = camera.to(device=DEV)
    for cfg, depth16 in ((RasterConfig(), False), (RasterConfig(), True), (RasterConfig(antialias=True, blur_cov=0.0), False)):
        gd = g.to(DEV).requires_grad_(True)
        r = gs.render_gaussians(gd, cam, cfg, use_sh=False, render_depth=True, use_depth16=depth16,
                                render_median_depth=True)
        ocfg = orc.OracleConfig.of(cfg)
        p_np, d_np = pu.to_np(r.gaussians2d), pu.to_np(r.point_depth)
        idx = pu.to_np(r.points_in_view)
        ndc = orc.ndc_depth(d_np, camera.near_plane, camera.far_plane)
        o2p, ranges = orc.map_to_tiles(p_np, ndc, size, ocfg, depth16)
        feats = np.concatenate([d_np, d_np ** 2, g.feature.numpy()[idx]], 1).astype(np.float32)
        image_ref, alpha_ref, _ = orc.rasterize_with_tiles(p_np, feats, o2p, ranges, size, ocfg)
        tol = dict(atol=2e-4, rtol=2e-4) if cfg.antialias else {}
        proof = pu.flip_proof(p_np, feats, o2p, ranges, size, ocfg,
                              bar=pu.AA_FLIP_MARGIN if cfg.antialias else pu.FLIP_MARGIN)
        pu.assert_pixels_close(r.image, image_ref[..., 2:], "image", flips=proof.channels(slice(2, None)), **tol)
        pu.assert_pixels_close(r.image_weight, alpha_ref, "weight", flips=proof.weight(), **tol)
        w = alpha_ref + np.float32(1e-6)
        pu.assert_pixels_close(r.depth, image_ref[..., 0] / w, "depth", atol=1e-3, rtol=1e-3, flips=proof.weight(),
                               bound=False)
        import dataclasses
        mcfg = orc.OracleConfig.of(dataclasses.replace(cfg, use_alpha_blending=False, saturate_threshold=0.5))
        med_ref, _, _ = orc.rasterize_with_tiles(p_np, d_np, o2p, ranges, size, mcfg)
        assert r.median_depth.shape == (size[1], size[0])
        pu.assert_pixels_close(r.median_depth, med_ref[..., 0], "median depth", atol=1e-4, rtol=1e-4,
                               flips=proof.weight(), bound=False)
        (r.image.sum() + r.depth.sum()).backward()
        assert gd.feature.grad.shape == g.feature.shape and bool(torch.isfinite(gd.position.grad).all())
        assert float(gd.feature.grad.abs().sum()) > 0


def test_float64_and_cpu_inputs_are_rejected_not_emulated():
    g, camera = scenes.benchmark_scene(100, (64, 64), sh_degree=1)
    cam = camera.to(device=DEV)
    with pytest.raises(TypeError, match="float32"):
        gs.render_gaussians(g.to(DEV).to(dtype=torch.float64), cam.to(dtype=torch.float64), RasterConfig(), use_sh=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        gs.render_gaussians(g, cam, RasterConfig(), use_sh=True)


# ------------------------------------------------------------------------- Morton ordering
def _morton_numpy(points, resolution, size=2 ** 20):
    """numpy restatement of reference misc/morton_sort.py:10-66, 91-99 (f32 cell arithmetic)"""
    p = points.astype(np.float32)
    lower = p.min(0)
    upper = (lower + np.float32(size * resolution)).astype(np.float32)
    inc = ((upper - lower) / np.float32(size)).astype(np.float32)[0]
    v = ((p - lower) / inc).astype(np.float32)
    cell = np.clip(v, 0, size - 1).astype(np.uint64)

    def spread(x):
        x = x & np.uint64(0x1fffff)
        x = (x | (x << np.uint64(32))) & np.uint64(0x1f00000000ffff)
        x = (x | (x << np.uint64(16))) & np.uint64(0x1f0000ff0000ff)
        x = (x | (x << np.uint64(8))) & np.uint64(0x100f00f00f00f00f)
        x = (x | (x << np.uint64(4))) & np.uint64(0x10c30c30c30c30c3)
        x = (x | (x << np.uint64(2))) & np.uint64(0x1249249249249249)
        return x
    return spread(cell[:, 0]) | (spread(cell[:, 1]) << np.uint64(1)) | (spread(cell[:, 2]) << np.uint64(2))


def test_morton_sort_bit_exact():
    from taichi_gaussian_rasterizer_amd.misc import morton_sort
    rng = np.random.default_rng(0)
    for n, res in ((1, 0.01), (1000, 0.001), (200000, 0.0005)):
        pts = (rng.standard_normal((n, 3)) * 3).astype(np.float32)
        codes = pu.to_np(morton_sort.morton_codes(dev(pts), res)).view(np.uint64)
        ref = _morton_numpy(pts, res)
        assert (codes == ref).all()
        order = pu.to_np(morton_sort.argsort(dev(pts), res))
        assert (order == np.argsort(ref, kind="stable")).all()
        assert torch.equal(morton_sort.sort(dev(pts), res), dev(pts[np.argsort(ref, kind="stable")]))
    d = morton_sort.argsort_dedup(dev(np.zeros((10, 3), np.float32)), 0.1)
    assert d.shape == (1,)


# ---------------------------------------------------------- skewed splat-size distribution
def test_mapper_and_raster_with_huge_and_tiny_splats():
    """real scenes mix sub-pixel splats with a few that cover most of the screen: exercises the
    mapper's outside-window path (splats reaching beyond their region's LDS window), long per-lane
    tile loops, crowded tiles (bitonic sort) and deep blend lists; results must still match the oracle
    bit for bit (mapper) / within tolerance (rasterizer)."""
    size, n = (640, 400), 6000
    rng = np.random.default_rng(7)
    mean = rng.random((n, 2)) * np.array(size)
    ang = rng.random(n) * 2 * np.pi
    axis = np.stack([np.cos(ang), np.sin(ang)], 1)
    sig = np.exp(rng.normal(1.0, 1.2, (n, 2)))                 # log-normal: 0.1 .. 100 px
    big = rng.choice(n, 60, replace=False)
    sig[big] = rng.uniform(80, 400, (60, 2))                   # 1 % cover large parts of the image
    alpha = rng.uniform(0.05, 0.9, (n, 1))
    g2d = np.concatenate([mean, axis, sig, alpha], 1).astype(np.float32)
    depth = rng.random((n, 1)).astype(np.float32)
    feat = rng.random((n, 3)).astype(np.float32)
    cfg = RasterConfig()
    ocfg = orc.OracleConfig.of(cfg)
    o2p_ref, ranges_ref = orc.map_to_tiles(g2d, depth, size, ocfg)
    o2p, ranges = gs.map_to_tiles(dev(g2d), dev(depth), size, cfg)
    assert (pu.to_np(ranges) == ranges_ref).all() and (pu.to_np(o2p) == o2p_ref).all()
    counts = (ranges_ref[..., 1] - ranges_ref[..., 0])
    assert counts.max() > 64 and o2p_ref.shape[0] > 5 * n       # deep lists, many overlaps per splat
    image_ref, alpha_ref, _ = orc.rasterize_with_tiles(g2d, feat, o2p_ref, ranges_ref, size, ocfg)
    g_t, f_t = dev(g2d).requires_grad_(True), dev(feat).requires_grad_(True)
    out = gs.rasterize_with_tiles(g_t, f_t, o2p, ranges.view(-1, 2), size, cfg)
    proof = pu.flip_proof(g2d, feat, o2p_ref, ranges_ref, size, ocfg)
    pu.assert_pixels_close(out.image, image_ref, "image", flips=proof)
    pu.assert_pixels_close(out.image_weight, alpha_ref, "alpha", flips=proof.weight())
    gi = torch.rand(size[1], size[0], 3, generator=torch.Generator().manual_seed(2))
    (out.image * dev(gi)).sum().backward()
    gg, gf, _ = orc.rasterize_backward(g2d, feat, o2p_ref, ranges_ref, size, pu.to_np(out.image), gi.numpy(), ocfg)
    # the stated bar (2e-4), with the f64 oracle as the yardstick where the two f32 results part (deep blend lists)
    _, gg64, gf64 = pu.raster_truth(g2d, feat, o2p_ref, ranges_ref, size, ocfg, gi)
    pu.assert_grad_close_vs_truth(g_t.grad, gg, gg64, "grad_gaussians2d")
    pu.assert_grad_close_vs_truth(f_t.grad, gf, gf64, "grad_features")


@pytest.mark.parametrize("nb", [1, 4])
def test_raster_needle_splats_across_many_tiles(nb, monkeypatch):
    """100:1 ... 600:1 splats (sigma 300 x 0.5 px) crossing the whole image: a sub-block hundreds of pixels from the mean
    along the long axis is reached only through a corridor one pixel wide.  The sub-block cull (gs_sub_block_mask) must
    form |t|^2 there without the (sigma1 / sigma2)^2 cancellation of the expanded quadratic; a dropped block shows up
    as missing pixels and missing gradient against the oracle, which evaluates every pixel of every listed tile."""
    from taichi_gaussian_rasterizer_amd import _native as nv
    monkeypatch.setitem(nv.TUNING, "wave_sub_blocks", int(nb))
    size, n, needles = (640, 400), 400, 60
    rng = np.random.default_rng(17)
    mean = rng.random((n, 2)) * np.array(size)
    ang = rng.random(n) * 2 * np.pi
    axis = np.stack([np.cos(ang), np.sin(ang)], 1)
    sig = rng.uniform(2.0, 12.0, (n, 2))
    sig[:needles] = np.stack([rng.uniform(150, 300, needles), rng.uniform(0.45, 1.5, needles)], 1)
    mean[:needles // 2] += np.array(size) * rng.choice([-0.6, 0.6], (needles // 2, 2))  # means far outside the image
    alpha = rng.uniform(0.3, 0.95, (n, 1))
    g2d = np.concatenate([mean, axis, sig, alpha], 1).astype(np.float32)
    depth = rng.random((n, 1)).astype(np.float32)
    feat = rng.random((n, 3)).astype(np.float32)
    cfg = RasterConfig()
    ocfg = orc.OracleConfig.of(cfg)
    o2p_ref, ranges_ref = orc.map_to_tiles(g2d, depth, size, ocfg)
    o2p, ranges = gs.map_to_tiles(dev(g2d), dev(depth), size, cfg)
    assert (pu.to_np(ranges) == ranges_ref).all() and (pu.to_np(o2p) == o2p_ref).all()
    image_ref, alpha_ref, _ = orc.rasterize_with_tiles(g2d, feat, o2p_ref, ranges_ref, size, ocfg)
    g_t, f_t = dev(g2d).requires_grad_(True), dev(feat).requires_grad_(True)
    out = gs.rasterize_with_tiles(g_t, f_t, o2p, ranges.view(-1, 2), size, cfg)
    proof = pu.flip_proof(g2d, feat, o2p_ref, ranges_ref, size, ocfg)
    pu.assert_pixels_close(out.image, image_ref, "image", flips=proof)
    pu.assert_pixels_close(out.image_weight, alpha_ref, "alpha", flips=proof.weight())
    gi = torch.rand(size[1], size[0], 3, generator=torch.Generator().manual_seed(18))
    (out.image * dev(gi)).sum().backward()
    gg, gf, _ = orc.rasterize_backward(g2d, feat, o2p_ref, ranges_ref, size, pu.to_np(out.image), gi.numpy(), ocfg)
    _, gg64, gf64 = pu.raster_truth(g2d, feat, o2p_ref, ranges_ref, size, ocfg, gi)
    pu.assert_grad_close_vs_truth(g_t.grad, gg, gg64, "grad_gaussians2d")
    pu.assert_grad_close_vs_truth(f_t.grad, gf, gf64, "grad_features")
    # the needles themselves, row by row (a normwise bar is dominated by the round splats)
    pu.assert_rows_close(g_t.grad[:needles], gg64[:needles], "needle rows", tol=2e-2, frac=0.95)


# ------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("n,size,scale,cfg_kw", [(200000, (1024, 768), 2.0, {}), (60000, (512, 384), 6.0, {}),
                                                 (20000, (256, 192), 6.0, dict(compute_visibility=True))])
def test_repeated_frames_are_identical(n, size, scale, cfg_kw):
    """the per-pixel blend order is fixed by the per-tile sort, so the image of a frame does not depend on the arrival
    order of any atomic: 25 renders of one frame (large grid; crowded tiles; small grid with 8x8 wave regions) are
    bit-identical, their gradients equal up to float summation order (tools/exp_soak.py runs the long version)"""
    g, camera = scenes.benchmark_scene(n, size, sh_degree=2, seed=2, scale_factor=scale)
    cam = camera.to(device=DEV)
    cfg = RasterConfig(**cfg_kw)
    a = g.to(DEV).requires_grad_(True)
    gi = dev(torch.rand(size[1], size[0], 3, generator=torch.Generator().manual_seed(4)))
    first = None
    for _ in range(25):
        for _, t in a.items():
            t.grad = None
        r = gs.render_gaussians(a, cam, cfg, use_sh=True)
        r.image.backward(gi)
        if first is None:
            first = (r.image.detach().clone(), r.points_in_view.clone(), {k: t.grad.clone() for k, t in a.items()})
            continue
        assert torch.equal(r.image, first[0]) and torch.equal(r.points_in_view, first[1])
        for k, t in a.items():
            pu.assert_grad_close(t.grad, first[2][k], f"repeat grad {k}", tol=1e-3)
