"""The MCMC strategy restated in numpy: the draw in exact integers, the correction series and the perturbation in
float64, relocate and grow composed from them on plain arrays.  What the kernels must equal (the draw, the copies,
every moved byte) or stay within a derived bound of (the float32 outputs)."""
import math

import numpy as np

N_MAX = 51
TOP = 1.0 - 2.0 ** -23
VALUE_TOL = 1e-6  # rtol = atol: one float32 rounding of the term plus one of the sum, about 2 ulp, times four


def quantise(weights, exclude=None):
    """q = floor(clamp(w, 0, 1) * 2^24) as uint64; NaN, negative and excluded rows give 0"""
    w = np.asarray(weights, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        clamped = np.where(w > 0, np.minimum(w, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    q = np.floor(clamped.astype(np.float64) * 2.0 ** 24).astype(np.uint64)  # exact: a float32 times a power of two
    if exclude is not None:
        q[np.asarray(exclude).astype(bool)] = 0
    return q


def scaled_draw(random, total: int):
    """floor(r * total / 2^32) for r < 2^32, total < 2^55, exactly, in uint64: with total = hi 2^32 + lo the product is
    r hi 2^32 + r lo, whose first term is a multiple of 2^32 and whose second stays below 2^64"""
    r = np.asarray(random, dtype=np.uint64)
    hi, lo = np.uint64(total >> 32), np.uint64(total & 0xffffffff)
    return r * hi + ((r * lo) >> np.uint64(32))


def reference_sample(weights, random, exclude=None, select=None):
    """-> (rows int32 (m,), copies int32 (n,)); random: integers in 0 .. 2^32 - 1"""
    q = quantise(weights, exclude)
    n, random = q.shape[0], np.asarray(random, dtype=np.uint64)
    m = random.shape[0]
    cum = np.cumsum(q, dtype=np.uint64)  # total < 2^55: exact in any order
    total = int(cum[-1]) if n else 0
    rows = np.arange(m, dtype=np.int64)
    drawn = np.ones(m, dtype=bool) if select is None else np.asarray(select).astype(bool)
    if total == 0:
        drawn = np.zeros(m, dtype=bool)
    t = scaled_draw(random[drawn], total)
    picked = np.searchsorted(cum, t, side="right")  # the first i with cum[i] > t
    assert (q[picked] > 0).all() and (picked < n).all()
    rows[drawn] = picked
    copies = np.bincount(picked, minlength=n).astype(np.int32)
    return rows.astype(np.int32), copies


def reference_values(opacity, log_scaling, copies, min_opacity=0.005):
    """the correction in float64 -> (alpha_logit float64 (n,), log_scaling float64 (n, 3)); rows with copies == 0
    keep log_scaling and get NaN for alpha_logit"""
    o = np.asarray(opacity, dtype=np.float32).reshape(-1).astype(np.float64)
    ls = np.asarray(log_scaling, dtype=np.float32).astype(np.float64)
    lo = float(np.float32(min_opacity))
    alpha, out = np.full(o.shape, np.nan), ls.copy()
    for row in np.nonzero(np.asarray(copies) > 0)[0]:
        n = min(int(copies[row]) + 1, N_MAX)
        x = min(max(1.0 - (1.0 - o[row]) ** (1.0 / n), lo), TOP)
        denom = 0.0
        for i in range(1, n + 1):
            for k in range(i):
                denom += math.comb(i - 1, k) * (-1) ** k * x ** (k + 1) / math.sqrt(k + 1)
        alpha[row] = math.log(x / (1.0 - x))
        out[row] = ls[row] + math.log(o[row] / denom)
    return alpha, out


def rotation_matrices(rotation):
    q = np.asarray(rotation, dtype=np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    return np.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y,
                     2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x,
                     2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y], axis=1).reshape(-1, 3, 3)


def reference_perturb(log_scaling, rotation, alpha_logit, noise, scale, k=100.0, x0=0.995):
    """float64 from the float32 inputs -> (d (n, 3), gate (n,), the gate's exponent k ((1 - o) - x0) (n,))"""
    a = np.asarray(alpha_logit, dtype=np.float64).reshape(-1)
    with np.errstate(over="ignore"):
        o = 1.0 / (1.0 + np.exp(-a))
        exponent = k * ((1.0 - o) - x0)
        g = 1.0 / (1.0 + np.exp(-exponent))
    s2 = np.exp(np.asarray(log_scaling, dtype=np.float64)) ** 2
    R = rotation_matrices(rotation)
    v = np.asarray(noise, dtype=np.float64) * (g * float(scale))[:, None]
    t = s2 * np.einsum("nji,nj->ni", R, v)
    return np.einsum("nij,nj->ni", R, t), g, exponent


def perturb_bound(log_scaling, noise, position, gate, scale):
    """per row: 1e-4 scale g max(s^2) |noise|_2 + 2^-23 |position|_inf"""
    s2 = np.exp(np.asarray(log_scaling, dtype=np.float64)).max(axis=1) ** 2
    first = 1e-4 * float(scale) * gate * s2 * np.linalg.norm(np.asarray(noise, dtype=np.float64), axis=1)
    return first, 2.0 ** -23 * np.abs(np.asarray(position, dtype=np.float64)).max(axis=1)


def reference_relocate(tensors, state, dead, random, min_opacity=0.005, mode="zero"):
    """tensors, state: name -> array (state: name -> key -> array), dead bool (n,), random (n,) integers.  opacity is
    taken from tensors['opacity'] (the caller's float32 sigmoid, not a table column).
    -> (new tensors with alpha_logit / log_scaling in float64, new state, src_of, copies)"""
    dead = np.asarray(dead).astype(bool)
    opacity = np.asarray(tensors["opacity"], dtype=np.float32).reshape(-1)
    src_of, copies = reference_sample(opacity, random, exclude=dead, select=dead)
    alpha, scaling = reference_values(opacity, tensors["log_scaling"], copies, min_opacity)
    drawn = copies > 0
    out = {name: np.array(t)[src_of] for name, t in tensors.items() if name != "opacity"}
    shape = out["alpha_logit"].shape
    corrected = drawn[src_of]
    out["alpha_logit"] = np.where(corrected.reshape(shape), alpha[src_of].reshape(shape),
                                  out["alpha_logit"].astype(np.float64))
    out["log_scaling"] = np.where(corrected[:, None], scaling[src_of], out["log_scaling"].astype(np.float64))
    zero = drawn | (dead & (src_of != np.arange(len(dead)))) if mode == "zero" else drawn  # moved rows and sources
    new_state = {}
    for name, table in state.items():
        new_state[name] = {}
        for key, t in table.items():
            t = np.array(t)
            t[zero] = 0
            new_state[name][key] = t
    return out, new_state, src_of, copies


def reference_grow(tensors, state, random, min_opacity=0.005):
    """count = len(random) rows appended -> (tensors, state, src_of (n + count,), copies (n,))"""
    opacity = np.asarray(tensors["opacity"], dtype=np.float32).reshape(-1)
    n, count = opacity.shape[0], len(random)
    drawn_rows, copies = reference_sample(opacity, random)
    src_of = np.concatenate([np.arange(n, dtype=np.int32), drawn_rows])
    alpha, scaling = reference_values(opacity, tensors["log_scaling"], copies, min_opacity)
    out = {name: np.array(t)[src_of] for name, t in tensors.items() if name != "opacity"}
    shape = out["alpha_logit"].shape
    corrected = (copies > 0)[src_of]
    out["alpha_logit"] = np.where(corrected.reshape(shape), alpha[src_of].reshape(shape),
                                  out["alpha_logit"].astype(np.float64))
    out["log_scaling"] = np.where(corrected[:, None], scaling[src_of], out["log_scaling"].astype(np.float64))
    new_state = {}
    for name, table in state.items():
        new_state[name] = {key: np.concatenate([np.array(t), np.zeros((count, *np.shape(t)[1:]), np.array(t).dtype)])
                           for key, t in table.items()}
    return out, new_state, src_of, copies
