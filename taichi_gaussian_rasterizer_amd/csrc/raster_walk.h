// raster_walk.h -- what the f32 rasterizers (raster_fwd.hip, raster_bwd.hip, raster_wide.hip) do alike around their
// per-splat walks, once: block -> pixel region, the launch geometry behind it, and a splat's row -> the LDS record the
// walk reads, so that the backward tests a pixel with the forward's own expression by construction.  The per-pixel
// arithmetic is raster_pdf.h (general mode) and the kernels' own (lean modes).  Everything inlines; what that leaves of
// the kernels' code: profiles/raster_walk/isa_identity.txt.
#pragma once

#include "gs_common.h"
#include "raster_pdf.h"

// ------------------------------------------------------------------ host: launch geometry
// forward_cut as the forward kernels use it.  Below 2^-25 (half an ulp of 1) the reference's own f32 accumulation
// W += w no longer changes W, but it still adds alpha * (1 - W) * feature for every remaining splat with 1 - W stuck at
// ~2^-24; the kernels carry T itself and stop here: forward_cut = 0 differs from the reference by
// < N * 2^-24 * max|feature| (N remaining splats)
static inline float gs_forward_cut(const GsRasterConfig* cfg) {
  return cfg->forward_cut > 2.98023223876953125e-08f ? cfg->forward_cut : 2.98023223876953125e-08f;
}
// The launch geometry of a narrow rasterizer call, and the wave's sub-block count in `nb`.  A shard that owns no tile
// row leaves num_tiles == 0 and nothing else: the caller returns GS_OK.
template <typename Args>
static inline int gs_raster_geometry(Args& a, const GsRasterConfig* cfg, int width, int height, const int32_t* tile_order,
                                     const int32_t* heavy_tiles, const GsRowShard* shard, int backward, int& nb) {
  const int ts = cfg->tile_size;
  a.tiles_wide = int(gs_div_up(width, ts));
  a.tile_size = ts;
  if (int rc = gs_make_shard(shard, int(gs_div_up(height, ts)), &a.sh)) return rc;
  a.num_tiles = a.tiles_wide * a.sh.local_rows;
  if (a.num_tiles == 0) return GS_OK;
  nb = gs_raster_sub_blocks(cfg, a.num_tiles, backward);
  a.sub_x = ts / (nb == 1 ? 8 : 16);
  a.sub_y = ts / (nb == 4 ? 16 : 8);
  a.num_items = a.num_tiles * a.sub_x * a.sub_y;
  a.tile_order = tile_order;
  // the split needs the 2x2-quadrant geometry of a 16-pixel tile and a launch order to index into
  a.heavy = (tile_order && ts == 16 && nb > 1) ? heavy_tiles : nullptr;
  a.heavy_cap = a.num_tiles / 4;
  if (cfg->tune_no_heavy_split) a.heavy = nullptr;
  return GS_OK;
}
// workgroups of a narrow launch: the regions, four more per tile that may be split, padded for gs_xcd_remap
template <typename Args>
static inline int gs_raster_grid(const Args& a) {
  return 8 * int(gs_div_up(a.num_items + (a.heavy ? 4 * a.heavy_cap : 0), 8));
}

#ifdef __HIPCC__
// ------------------------------------------------------------------ device: block -> region
template <int N> struct GsInt { static constexpr int value = N; };
// (column, row) of a tile in a grid `tiles_wide` across
__device__ __forceinline__ void gs_tile_col_row(int tile, int tiles_wide, int& tx, int& ty) {
  ty = tile / tiles_wide;
  tx = tile - ty * tiles_wide;
}
// pixel origin of a (local) tile in the full image, and the row of the image buffers it starts at
template <typename Args>
__device__ __forceinline__ void gs_tile_origin(const Args& a, int tile, int& x0, int& y0, int& yout0) {
  int tx, lty;
  gs_tile_col_row(tile, a.tiles_wide, tx, lty);
  x0 = tx * a.tile_size;
  y0 = gs_shard_global_row(a.sh, lty) * a.tile_size;
  yout0 = lty * a.tile_size;
}

// Block -> work of the narrow kernels: body(GsInt<sub-blocks>, tile, x0, y0, yout0) is called for the region this
// workgroup owns, if it owns one.  With a launch order from the mapper: its first `*heavy` tiles (the fullest ones;
// tile_size 16 only) are rasterized by FOUR workgroups each, one per 8x8 quadrant, the others by workgroups of the grid's
// own wave region -- a launch cannot end before its fullest tile has been walked by one wave, which is what bounds small
// grids (strips of a sharded frame, training-size images).  Without an order: XCD-contiguous bands.
// (A callback: with a returned region for the kernel to branch on, the compiler lays out both files anew.)
template <int NB, typename Args, typename Body>
__device__ __forceinline__ void gs_raster_region(const Args& a, Body body) {
  const int per_tile = a.sub_x * a.sub_y;
  constexpr int RW = NB == 1 ? 8 : 16, RH = NB == 4 ? 16 : 8;  // the wave's pixel region: NB 8x8 sub-blocks
  int tile, quad;
  if (a.tile_order) {
    const int b = blockIdx.x;
    const int heavy = (NB > 1 && a.heavy) ? min(*a.heavy, a.heavy_cap) : 0;
    if (NB > 1 && b < 4 * heavy) {
      tile = a.tile_order[b >> 2];
      int x0, y0, yout0;
      gs_tile_origin(a, tile, x0, y0, yout0);
      x0 += (b & 1) * 8; y0 += ((b >> 1) & 1) * 8; yout0 += ((b >> 1) & 1) * 8;
      if (x0 < a.W && y0 < a.H) body(GsInt<1>{}, tile, x0, y0, yout0);
      return;
    }
    const int c = b - 4 * heavy, rank = heavy + c / per_tile;
    if (rank >= a.num_tiles) return;
    tile = a.tile_order[rank];
    quad = c % per_tile;
  } else {
    const int item = gs_xcd_remap(blockIdx.x, a.num_items);
    if (item < 0) return;
    tile = item / per_tile;
    quad = item - tile * per_tile;
  }
  int x0, y0, yout0;
  gs_tile_origin(a, tile, x0, y0, yout0);
  x0 += (quad % a.sub_x) * RW; y0 += (quad / a.sub_x) * RH; yout0 += (quad / a.sub_x) * RH;
  if (x0 >= a.W || y0 >= a.H) return;
  body(GsInt<NB>{}, tile, x0, y0, yout0);
}

// the wide kernels' (no launch order, no shard, 8x8 regions): false for a padding block or a region outside the image
template <typename Args>
__device__ __forceinline__ bool gs_wide_region(const Args& a, int& tile, int& x0, int& y0) {
  const int item = gs_xcd_remap(blockIdx.x, a.num_items);
  if (item < 0) return false;
  const int per_tile = a.side * a.side;
  tile = item / per_tile;
  const int q = item - tile * per_tile;
  int tx, ty;
  gs_tile_col_row(tile, a.tiles_wide, tx, ty);
  x0 = tx * a.tile_size + (q % a.side) * 8;
  y0 = ty * a.tile_size + (q / a.side) * 8;
  return x0 < a.W && y0 < a.H;
}

// ------------------------------------------------------------------ device: a splat's staged record: GEO_V4 float4s
// of geometry followed by the feature row (one LDS address, b128 reads)
// feature row (F floats, padded to FP with zeros) -> the record's float4 words (the backward's: see raster_fwd.hip)
template <int FP, int GEO_V4>
__device__ __forceinline__ void gs_stage_features(float4* rec, const float* f, int F) {
#pragma unroll
  for (int q = 0; q < (FP + 3) / 4; ++q) {
    float fv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) fv[k] = (4 * q + k < FP && 4 * q + k < F) ? f[4 * q + k] : 0.0f;
    rec[GEO_V4 + q] = make_float4(fv[0], fv[1], fv[2], fv[3]);
  }
}
// ... and back into registers
template <int FP, int GEO_V4>
__device__ __forceinline__ void gs_fetch_features(const float4* rec, float (&feat)[FP]) {
#pragma unroll
  for (int q = 0; q < (FP + 3) / 4; ++q) {
    const float4 fq = rec[GEO_V4 + q];
    const float fv[4] = {fq.x, fq.y, fq.z, fq.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (4 * q + k < FP) feat[4 * q + k] = fv[k];
  }
}

// a row of `points` (mean, axis, the two sigmas, opacity) and the sigmas' reciprocals (v_rcp_f32: 1 ulp, far inside the
// parity tolerance)
struct GsSplat { float mx, my, ax, ay, sx, sy, al, isx, isy; };
__device__ __forceinline__ GsSplat gs_load_splat(const float* p) {
  return {p[0], p[1], p[2], p[3], p[4], p[5], p[6], gs_rcp_fast(p[4]), gs_rcp_fast(p[5])};
}

constexpr float GS_K_EXP = 0.84932180028801904f;  // sqrt(0.5 * log2(e)): exp(-0.5 t^2) = exp2(-(k t)^2)

// the ellipse frame t = (A . d, B . d), d = pixel - mean, scaled by ks
struct GsEllipseFrame { float Ax, Ay, Bx, By; };
__device__ __forceinline__ GsEllipseFrame gs_splat_frame(const GsSplat& s, float ks) {
  return {s.ax * s.isx * ks, s.ay * s.isx * ks, -s.ay * s.isy * ks, s.ax * s.isy * ks};
}

// The geometry words: each function writes them to `rec` and returns the conservative mask of the region's NB sub-blocks
// that the splat can reach (gs_common.h); (x0, y0) is the region's first pixel.
//
// Lean (narrow forward and backward alike): the frame scaled by K_EXP so that alpha = exp2(-(tx^2 + ty^2 + g1.z)) with
// g1.z = -log2(opacity): it starts the exponent's fma chain, so v_exp_f32 returns alpha itself.  The ellipse-frame
// coordinates of a pixel are tx = A . (X - m) = A . (X - origin) + A . (origin - m): the second term is formed once per
// (region, splat) here, and a pixel's tx is two fma on its origin-relative centre (|X - origin| < 16: no cancellation
// beyond what X - m has) instead of two subtractions, a multiply and an fma.
template <int NB>
__device__ __forceinline__ int gs_stage_lean(float4* rec, const GsSplat& s, int x0, int y0, float thr, float inv_thr) {
  const GsEllipseFrame f = gs_splat_frame(s, GS_K_EXP);
  int mask = 0;
  if (s.al > thr)  // alpha * exp2(-(tx^2 + ty^2)) > thr needs tx^2 + ty^2 < log2(alpha / thr)
    mask = gs_sub_block_mask<NB>(f.Ax, f.Ay, f.Bx, f.By, __log2f(s.al * inv_thr), float(x0) + 0.5f - s.mx,
                                 float(y0) + 0.5f - s.my);
  const float ox = float(x0) - s.mx, oy = float(y0) - s.my;
  rec[0] = make_float4(__builtin_fmaf(f.Ax, ox, f.Ay * oy), __builtin_fmaf(f.Bx, ox, f.By * oy), f.Ax, f.Ay);
  rec[1] = make_float4(f.Bx, f.By, -__log2f(s.al), __int_as_float(mask));
  return mask;
}

// General (narrow MODE 2 and the wide kernels; raster_pdf.h): g0 = (mean, A), g1 = (B, opacity, mask), g2 = (axis,
// 1 / sigma), the mean absolute; the mask word only where `mask_word` says so (the narrow kernels).  Forward: the frame
// scaled by K_EXP.  Backward: unscaled; and for the antialiased pdf, whose per-pixel code works in the splat's frame
// (ux, uy) and needs the sigmas and the half pixel in sigma units, g0 = (mean, sx, sy), g1 = (.5 / sx, .5 / sy, ..).
template <int NB, bool BWD>
__device__ __forceinline__ int gs_stage_general(float4* rec, const GsSplat& s, int x0, int y0, float thr, float inv_thr,
                                                int aa, bool mask_word) {
  const GsEllipseFrame f = gs_splat_frame(s, BWD ? 1.0f : GS_K_EXP);
  int mask = 0;
  if (aa) {
    float d0x, d0y;  // D(0; s) = S(0.5 / s) - S(-0.5 / s) = 2 S(0.5 / s) - 1, each direction in its own form
    if (BWD) {
      float s1, s2, u0, u1;
      s_sig_grad(0.5f, s.isx, s1, u0, u1);
      s_sig_grad(0.5f, s.isy, s2, u0, u1);
      d0x = 2.0f * s1 - 1.0f; d0y = 2.0f * s2 - 1.0f;
    } else {
      d0x = s_sig(0.5f, s.isx) - s_sig(-0.5f, s.isx); d0y = s_sig(0.5f, s.isy) - s_sig(-0.5f, s.isy);
    }
    mask = gs_sub_block_mask_antialias<NB>(s.ax, s.ay, s.sx, s.sy, s.al, inv_thr, d0x, d0y, float(x0) + 0.5f - s.mx,
                                           float(y0) + 0.5f - s.my);
  } else if (s.al > thr) {
    // alpha * pdf > thr  needs  tx^2 + ty^2 < log2(alpha / thr)  (scaled frame; 2 ln(alpha / thr) unscaled)
    const float r2 = __log2f(s.al * inv_thr) * (BWD ? 1.38629436111989f : 1.0f);
    mask = gs_sub_block_mask<NB>(f.Ax, f.Ay, f.Bx, f.By, r2, float(x0) + 0.5f - s.mx, float(y0) + 0.5f - s.my);
  }
  const float mw = mask_word ? __int_as_float(mask) : 0.0f;
  if (BWD && aa) {
    rec[0] = make_float4(s.mx, s.my, s.sx, s.sy);
    rec[1] = make_float4(0.5f * s.isx, 0.5f * s.isy, s.al, mw);
  } else {
    rec[0] = make_float4(s.mx, s.my, f.Ax, f.Ay);
    rec[1] = make_float4(f.Bx, f.By, s.al, mw);
  }
  rec[2] = make_float4(s.ax, s.ay, s.isx, s.isy);
  return mask;
}

#endif  // __HIPCC__
