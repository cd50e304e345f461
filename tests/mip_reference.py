"""References for the Mip-Splatting entry points (csrc/mip.hip), on the CPU in numpy.

reference_sampling_rate   gs_mip_sampling_rate restated in float32, operation for operation: bit-exact by contract.
smooth3d / smooth3d_grad  the smoothing and its analytic gradients in the stable forms of the kernel, in the dtype asked
                          for: float64 is the truth the tests compare with, float32 the yardstick of their tolerances
                          (what the same formulas give when every operation rounds to float32).
smooth3d_naive_torch      the formulas as the contract states them, in torch: for autograd and for the benchmark."""
import numpy as np
import torch

CAMERA_FLOATS = 24


def pack_camera(T_camera_world, projection, image_size, near, far, margin=0.15):
    """one record of the packed table from plain numbers, as mip.pack_cameras builds it"""
    row = np.zeros(CAMERA_FLOATS, dtype=np.float32)
    row[0:12] = np.asarray(T_camera_world, dtype=np.float32)[:3].reshape(12)
    row[12:16] = np.asarray(projection, dtype=np.float32)
    m, one = np.float32(margin), np.float32(1)
    w, h = np.float32(image_size[0]), np.float32(image_size[1])
    row[16:20] = (-m * w, (one + m) * w, -m * h, (one + m) * h)
    row[20], row[21], row[22] = near, far, max(row[12], row[13])
    return row


def reference_sampling_rate(points, table):
    """points (N, 3) float32, table (C, 24) float32 -> (rate (N,) float32, seen (N,) int32)"""
    points, table = np.asarray(points), np.asarray(table)
    assert points.dtype == np.float32 and table.dtype == np.float32 and table.shape[1:] == (CAMERA_FLOATS,)
    px, py, pz = points[:, 0], points[:, 1], points[:, 2]
    rate = np.zeros(points.shape[0], dtype=np.float32)
    seen = np.zeros(points.shape[0], dtype=np.int32)
    with np.errstate(all="ignore"):
        for cam in table:
            xc = ((cam[0] * px + cam[1] * py) + cam[2] * pz) + cam[3]
            yc = ((cam[4] * px + cam[5] * py) + cam[6] * pz) + cam[7]
            zc = ((cam[8] * px + cam[9] * py) + cam[10] * pz) + cam[11]
            u = cam[12] * xc + cam[14] * zc
            v = cam[13] * yc + cam[15] * zc
            valid = ((zc >= cam[20]) & (zc <= cam[21]) & (cam[16] * zc <= u) & (u <= cam[17] * zc) &
                     (cam[18] * zc <= v) & (v <= cam[19] * zc))
            assert xc.dtype == np.float32 and u.dtype == np.float32
            ratio = (cam[22] / zc).astype(np.float32)
            rate = np.where(valid, np.maximum(rate, ratio), rate)
            seen += valid
    return rate, seen


def reference_filter_3d(rate, seen, variance=0.2):
    size = np.zeros_like(rate)
    visible = seen > 0
    if visible.any():
        size[visible] = np.float32(np.sqrt(variance)) / rate[visible]
        size[~visible] = size[visible].max()
    return size


def _terms(l, f):
    """per axis l', 1 / (1 + x), x / (1 + x), and log c; l (N, 3), f (N,) of one dtype"""
    one, half, two = (l.dtype.type(v) for v in (1, 0.5, 2))
    f = f[:, None]
    with np.errstate(all="ignore"):
        t = f * np.exp(-l)
        x = t * t
        small = x <= one
        L_small = np.log1p(x)
        r_small = one / (one + x)
        y = one / x
        w = np.log1p(y)
        s_big = one / (one + y)
        lp = np.where(small, l + half * L_small, np.log(f) + half * w)
        L = np.where(small, L_small, two * np.log(t) + w)
        r = np.where(small, r_small, y * s_big)
        s = np.where(small, x * r_small, s_big)
        log_c = -half * ((L[:, 0] + L[:, 1]) + L[:, 2])
    assert lp.dtype == l.dtype and log_c.dtype == l.dtype
    return lp, r, s, log_c


def smooth3d(l, a, f, dtype=np.float64):
    """(l', a', log c) of l (N, 3), a (N,), f (N,) >= 0 in `dtype`; rows with f == 0 are returned as they are"""
    l, a, f = (np.asarray(v).astype(dtype) for v in (l, a, f))
    one = dtype(1)
    lp, _, _, log_c = _terms(l, f)
    with np.errstate(all="ignore"):
        omc = -np.expm1(log_c)
        q = np.exp(a) * omc
        ap = np.where(q <= one, (a + log_c) - np.log1p(q), log_c - np.log(np.exp(-a) + omc))
    same = f == 0
    lp[same], ap[same], log_c[same] = l[same], a[same], 0
    assert ap.dtype == dtype
    return lp, ap, log_c


def smooth3d_grad(l, a, f, gl, ga, dtype=np.float64):
    """(dL/dl (N, 3), dL/da (N,)) from the gradients gl (N, 3), ga (N,) of the outputs, analytically, in `dtype`"""
    l, a, f, gl, ga = (np.asarray(v).astype(dtype) for v in (l, a, f, gl, ga))
    one = dtype(1)
    _, r, s, log_c = _terms(l, f)
    with np.errstate(all="ignore"):
        omc = -np.expm1(log_c)
        e, em = np.exp(a), np.exp(-a)
        q1, den = one + e * omc, em + omc
        low = a <= 0
        inv_rest = np.where(low, (one + e) / q1, (em + one) / den)
        da_da = np.where(low, one / q1, em / den)
        dl = gl * r + (ga * inv_rest)[:, None] * s
        da = ga * da_da
    same = f == 0
    dl[same], da[same] = gl[same], ga[same]
    assert dl.dtype == dtype and da.dtype == dtype
    return dl, da


def smooth3d_naive_torch(log_scaling, alpha_logit, filter3d):
    """the contract's formulas written plainly in torch (differentiable; accurate at moderate inputs only)"""
    f2 = filter3d.reshape(-1, 1) ** 2
    scale2 = torch.exp(2 * log_scaling)
    new_log_scaling = 0.5 * torch.log(scale2 + f2)
    c = torch.sqrt(torch.prod(scale2 / (scale2 + f2), dim=1)).reshape(alpha_logit.shape)
    opacity = torch.sigmoid(alpha_logit) * c
    return new_log_scaling, torch.log(opacity / (1 - opacity))


def smooth_inputs(n, domain, seed):
    """rows of a test domain: "moderate" l in [-7, 2], a in [-6, 6], f in {0} u [e^-8, e];
    "wide" |l|, |a| <= 40, f in {0} u [1e-12, 1e6] (log-uniform); every 7th row has f = 0.  float32 values."""
    rng = np.random.default_rng(seed)
    if domain == "moderate":
        l, a = rng.uniform(-7, 2, (n, 3)), rng.uniform(-6, 6, n)
        f = np.exp(rng.uniform(-8, 1, n))
    else:
        l, a = rng.uniform(-40, 40, (n, 3)), rng.uniform(-40, 40, n)
        f = np.exp(rng.uniform(np.log(1e-12), np.log(1e6), n))
    f[::7] = 0
    return l.astype(np.float32), a.astype(np.float32), f.astype(np.float32)


def forward_units(l, a, lp, ap, log_c):
    """the error units of the forward: 2^-24 (|l| + |l'| + 1) and 2^-24 (|a| + |log c| + |a'| + 1), from float64 values"""
    eps = 2.0 ** -24
    return eps * (np.abs(l) + np.abs(lp) + 1), eps * (np.abs(a) + np.abs(log_c) + np.abs(ap) + 1)


def backward_units(gl, ga):
    """the error units of the gradients: 2^-24 (|g_l| + 2 |g_a|) per axis and 2^-24 |g_a|"""
    eps = 2.0 ** -24
    return eps * (np.abs(gl) + 2 * np.abs(ga)[:, None]), eps * np.abs(ga)
