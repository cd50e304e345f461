// raster_pdf.h -- the general mode's per-pixel arithmetic (plain pdf taichi_lib/generic.py:321-336, antialiased pdf
// :341-404) and the antialiased pdf's pieces, shared by the narrow (raster_fwd.hip, raster_bwd.hip: MODE 2) and the
// wide-feature (raster_wide.hip) rasterizers.
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

// The antialiased pdf's sigmoid a = S(z) = 1 / (1 + exp(-(1.6 z + 0.07 z^3))) (taichi_lib/generic.py:341-369) and its
// derivative dS/dz = (1.6 + 0.21 z^2) S (1 - S), the log2(e) factors folded into the polynomial (S (1 - S) as a (1 - a),
// not e a^2: far out in the tail e overflows to inf while a is an exact 0), in two halves: the value alone decides
// whether a pixel takes anything from the splat; the derivative is only formed for the pixels that do (raster_bwd.hip:
// under their EXEC mask, skipped when the sub-block has none)
__device__ __forceinline__ float s_sig_value(float z) {
  const float e = gs_exp2_fast(z * __builtin_fmaf(-0.07f * 1.44269504088896341f, z * z, -1.6f * 1.44269504088896341f));
  return gs_rcp_fast(1.0f + e);
}
__device__ __forceinline__ float s_sig_slope(float z, float a) {
  return __builtin_fmaf(0.21f, z * z, 1.6f) * (a * (1.0f - a));
}

// ---- General mode (MODE 2 of raster_fwd.hip / raster_bwd.hip, and raster_wide.hip): the per-pixel arithmetic on a
// staged record g0, g1, g2 (gs_stage_general, raster_walk.h) at (dx, dy) = pixel centre - mean; `aa` (the antialiased
// pdf) is wave-uniform.  Forward: alpha = opacity * pdf
__device__ __forceinline__ float gs_general_alpha(int aa, float dx, float dy, const float4& g0v, const float4& g1v,
                                                  const float4& g2v) {
  if (aa) {
    // taichi_lib/generic.py:347-357
    const float tx = dx * g2v.x + dy * g2v.y, ty = dy * g2v.x - dx * g2v.y;
    float nx, dx_, ny, dy_;
    aa_axis(tx, g2v.z, nx, dx_);
    aa_axis(ty, g2v.w, ny, dy_);
    // tau sx sy D(tx) D(ty); sx sy = 1 / (isx isy) goes into the same reciprocal
    return g1v.z * (6.28318530717958648f * nx * ny * gs_rcp_fast(dx_ * dy_ * g2v.z * g2v.w));
  }
  const float tx = dx * g0v.z + dy * g0v.w, ty = dx * g1v.x + dy * g1v.y;
  return g1v.z * gs_exp2_fast(-(tx * tx + ty * ty));
}

// Backward.  The pdf's derivatives at one pixel are the caller's own scalars, dmx .. dsy = d pdf / d (mean, axis, sigma)
// and, with antialias, Px, Py = d pdf / d (ux, uy); aa_z, aa_a are the antialiased pdf's sigmoid arguments and values.
// (Scalars one by one: with a struct or an array of them the MODE 2 kernels take more registers.)
// The plain pdf and its derivatives (taichi_lib/generic.py:321-336) from the unscaled record g0 = (mean, A),
// g1 = (B, ..), g2 = (axis, 1 / sigma); tx, ty: the pixel in the ellipse frame.  Formed in front of the hit test.
__device__ __forceinline__ float gs_general_pdf_plain(float dx, float dy, const float4& g0v, const float4& g1v,
                                                      const float4& g2v, float& tx, float& ty, float& dmx, float& dmy,
                                                      float& dax, float& day, float& dsx, float& dsy) {
  tx = dx * g0v.z + dy * g0v.w; ty = dx * g1v.x + dy * g1v.y;
  const float p = gs_exp2_fast(-0.72134752044448170f * (tx * tx + ty * ty));
  const float txs = tx * g2v.z, tys = ty * g2v.w;
  dsx = tx * tx * p * g2v.z; dsy = ty * ty * p * g2v.w;
  dax = p * (txs * -dx + tys * -dy); day = p * (txs * -dy + tys * dx);
  dmx = p * (txs * g2v.x - tys * g2v.y); dmy = p * (txs * g2v.y + tys * g2v.x);
  return p;
}

// The antialiased pdf (taichi_lib/generic.py:341-404) in the splat's frame: u = R(axis) d, pdf = tau fx(ux) fy(uy) with
// f(u; s) = s (S((u + .5) / s) - S((u - .5) / s)).  With a_k = S(z_k), d_k = S'(z_k), z_1,2 = (u +- .5) / s:
//   df/du = d_1 - d_2,   df/ds = (a_1 - a_2) - (z_1 d_1 - z_2 d_2)
// record: g0 = (mean, sx, sy), g1 = (.5 / sx, .5 / sy, alpha, mask), g2 = (axis, 1 / sx, 1 / sy).
// Its value half -- aa_z = (zx_1, zx_2, zy_1, zy_2), aa_a = S(aa_z), pdf = tau (sx (a_0 - a_1)) (sy (a_2 - a_3)) -- is
// written out in raster_bwd.hip and raster_wide.hip: as a function the narrow MODE 2 kernels take more registers
// (profiles/raster_walk/isa_identity.txt).  These are the derivatives, for the pixels that passed the hit test.  dmx,
// dmy: the wave totals of aag Px, aag Py are rotated out of the frame once per splat (gs_mean_grad_from_splat_frame)
__device__ __forceinline__ void gs_general_pdf_gradient(float dx, float dy, const float4& g0v, const float (&aa_z)[4],
                                                        const float (&aa_a)[4], float& Px, float& Py, float& dax,
                                                        float& day, float& dsx, float& dsy) {
  const float d0 = s_sig_slope(aa_z[0], aa_a[0]), d1 = s_sig_slope(aa_z[1], aa_a[1]);
  const float d2 = s_sig_slope(aa_z[2], aa_a[2]), d3 = s_sig_slope(aa_z[3], aa_a[3]);
  const float Dx = aa_a[0] - aa_a[1], Dy = aa_a[2] - aa_a[3];
  const float tau = 6.28318530717958648f;
  const float fxt = tau * (g0v.z * Dx), fyt = tau * (g0v.w * Dy);
  Px = (d0 - d1) * fyt;
  Py = fxt * (d2 - d3);
  dsx = (Dx - __builtin_fmaf(aa_z[0], d0, -(aa_z[1] * d1))) * fyt;
  dsy = fxt * (Dy - __builtin_fmaf(aa_z[2], d2, -(aa_z[3] * d3)));
  dax = __builtin_fmaf(Px, dx, Py * dy);
  day = __builtin_fmaf(Px, dy, -(Py * dx));
}

// What a hit pixel contributes to the splat's nine sums (backward.py:184-198): the gradients of the mean (in the splat
// frame with antialias), axis, sigmas and opacity, and with `heur` the two densification heuristics.  ACC: added to S
// (the narrow kernel sums over its sub-blocks), or stored (the wide kernel has one pixel per lane).
template <bool ACC>
__device__ __forceinline__ void gs_general_sums(int aa, int heur, const float4& g1v, const float4& g2v, float p,
                                                float& dmx, float& dmy, float dax, float day, float dsx, float dsy,
                                                float Px, float Py, float alpha_grad, float* S) {
  auto put = [](float& s, float x) { s = ACC ? s + x : x; };
  const float aag = g1v.z * alpha_grad;  // :184
  if (aa) {
    put(S[0], aag * Px); put(S[1], aag * Py);  // splat frame; see the epilogue
    if (heur) {
      dmx = -Px * g2v.x + Py * g2v.y;
      dmy = -Px * g2v.y - Py * g2v.x;
    }
  } else {
    put(S[0], aag * dmx); put(S[1], aag * dmy);
  }
  put(S[2], aag * dax); put(S[3], aag * day);
  put(S[4], aag * dsx); put(S[5], aag * dsy);
  put(S[6], p * alpha_grad);
  if (heur) {
    put(S[7], aag * aag);                                  // :194-198
    put(S[8], fabsf(aag * dmx) + fabsf(aag * dmy));
  }
}

// the antialiased mean's gradient out of the splat frame: d ux / d mean = -axis, d uy / d mean = -perp(axis)
__device__ __forceinline__ void gs_mean_grad_from_splat_frame(float& g0, float& g1, float ax, float ay) {
  const float m0 = -g0 * ax + g1 * ay, m1 = -g0 * ay - g1 * ax;
  g0 = m0; g1 = m1;
}
