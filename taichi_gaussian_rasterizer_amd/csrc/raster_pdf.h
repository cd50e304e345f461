// raster_pdf.h -- the antialiased pdf's per-pixel pieces (taichi_lib/generic.py:341-404), shared by the narrow
// (raster_fwd.hip, raster_bwd.hip) and the wide-feature (raster_wide.hip) rasterizers.
#pragma once

#include "gs_common.h"

// S(z) = 1 / (1 + exp(-(1.6 z + 0.07 z^3))) at z = x / sigma
__device__ __forceinline__ float s_sig(float x, float inv_sigma) {
  const float z = x * inv_sigma;
  const float e = -1.6f * z - 0.07f * z * z * z;
  return gs_rcp_fast(1.0f + gs_exp2_fast(e * 1.44269504088896341f));
}

// One axis of the antialiased pdf (taichi_lib/generic.py:341-357): D(t) = S((t + 0.5) / s) - S((t - 0.5) / s) with
// S(z) = 1 / (1 + e(z)), e(z) = exp(-(1.6 z + 0.07 z^3)), returned as num / den = (e_b - e_a) / ((1 + e_a)(1 + e_b)) so
// that both axes share ONE reciprocal.  D is even (S(-z) = 1 - S(z)), so |t| is used: a >= 0 keeps e_a <= 1, and b is
// clamped at -5, where S(b) < 5e-8 (e_b stays below 2e7: no overflow in the product of the two axes).
__device__ __forceinline__ void aa_axis(float t, float inv_sigma, float& num, float& den) {
  const float u = fabsf(t);
  const float za = (u + 0.5f) * inv_sigma, zb = fmaxf((u - 0.5f) * inv_sigma, -5.0f);
  const float c1 = -1.6f * 1.44269504088896341f, c3 = -0.07f * 1.44269504088896341f;
  const float ea = gs_exp2_fast(za * (c1 + c3 * za * za)), eb = gs_exp2_fast(zb * (c1 + c3 * zb * zb));
  num = eb - ea;
  den = (1.0f + ea) * (1.0f + eb);
}

__device__ __forceinline__ void s_sig_grad(float x, float inv_sigma, float& s, float& ds_dx, float& ds_dsig) {
  // taichi_lib/generic.py:360-369
  const float z = x * inv_sigma;
  s = gs_rcp_fast(1.0f + gs_exp2_fast((-1.6f * z - 0.07f * z * z * z) * 1.44269504088896341f));
  const float d = (1.6f + 0.21f * z * z) * s * (1.0f - s);
  ds_dx = d * inv_sigma;
  ds_dsig = ds_dx * -z;
}

// The antialiased pdf's sigmoid S(z) = 1 / (1 + exp(-(1.6 z + 0.07 z^3))) (taichi_lib/generic.py:341-369) and its
// derivative in 15 issue slots: a = S(z), d = dS/dz = (1.6 + 0.21 z^2) S (1 - S); the log2(e) factors are folded into
// the polynomial.  (S (1 - S) as a (1 - a), not e a^2: far out in the tail e overflows to inf while a is an exact 0.)
__device__ __forceinline__ void s_sig_parts(float z, float& a, float& d) {
  const float z2 = z * z;
  const float e = gs_exp2_fast(z * __builtin_fmaf(-0.07f * 1.44269504088896341f, z2, -1.6f * 1.44269504088896341f));
  a = gs_rcp_fast(1.0f + e);
  d = __builtin_fmaf(0.21f, z2, 1.6f) * (a * (1.0f - a));
}
// ... in two halves: the value alone decides whether a pixel takes anything from the splat; the derivative is only
// formed for the pixels that do (raster_bwd.hip: under their EXEC mask, skipped when the sub-block has none)
__device__ __forceinline__ float s_sig_value(float z) {
  const float e = gs_exp2_fast(z * __builtin_fmaf(-0.07f * 1.44269504088896341f, z * z, -1.6f * 1.44269504088896341f));
  return gs_rcp_fast(1.0f + e);
}
__device__ __forceinline__ float s_sig_slope(float z, float a) {
  return __builtin_fmaf(0.21f, z * z, 1.6f) * (a * (1.0f - a));
}
