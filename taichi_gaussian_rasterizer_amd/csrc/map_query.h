// map_query.h -- what every unit of the tile mapper shares: the tile-overlap query (reference
// taichi_lib/grid_query.py:10-91), the depth part of the sort key (mapper/tile_mapper.py:34-59), the call's arguments
// and the workgroup scans.  Included by mapper.hip (the fused path), tile_sort.hip (the per-tile sorts) and
// map_reference.hip (the reference-shaped primitives).
//
// EVERY UNIT THAT INCLUDES THIS IS COMPILED WITH -ffp-contract=off.  Every f32 operation of the grid query is a single
// correctly rounded IEEE op in the same order as oracle/gsplat_oracle.cpp (the square roots through gs_det_sqrtf:
// hipcc's __fsqrt_rn is the 1-ulp native instruction), and the logarithm is gs_det_logf (include/gs_detmath.h), so the
// integer results -- which tiles a splat touches, the sort keys, the order inside every tile -- are bit-identical to the
// CPU oracle.
#pragma once

#include "gs_common.h"
#include "../../include/gs_detmath.h"

namespace {

struct GridQuery {
  float ib00, ib01, ib10, ib11;
  float rel_min_x, rel_min_y;
  int min_tx, min_ty, span_x, span_y;
};

// taichi_lib/grid_query.py:73-91 (obb_grid_query) + :10-27 (tile_ranges)
__device__ __forceinline__ GridQuery grid_query(const float* g, int Wp, int Hp, int tile_size, float alpha_thr) {
  GridQuery q;
  const float mx = g[0], my = g[1], ax = g[2], ay = g[3], sgx = g[4], sgy = g[5], alpha = g[6];
  if (!(alpha > alpha_thr)) {  // explicit cull; the reference yields NaN bounds here (SURVEY 8a')
    q.ib00 = q.ib01 = q.ib10 = q.ib11 = q.rel_min_x = q.rel_min_y = 0.f;
    q.min_tx = q.min_ty = q.span_x = q.span_y = 0;
    return q;
  }
  const float gscale = gs_det_sqrtf(2.0f * gs_det_logf(__fdiv_rn(alpha, alpha_thr)));
  const float sx = sgx * gscale, sy = sgy * gscale;
  const float a2x = -ay, a2y = ax;
  const float v1x = ax * sx, v1y = ay * sx, v2x = a2x * sy, v2y = a2y * sy;
  const float ex = gs_det_sqrtf(v1x * v1x + v2x * v2x), ey = gs_det_sqrtf(v1y * v1y + v2y * v2y);
  const float lox = mx - ex, loy = my - ey, hix = mx + ex, hiy = my + ey;
  q.ib00 = __fdiv_rn(ax, sx); q.ib01 = __fdiv_rn(ay, sx); q.ib10 = __fdiv_rn(a2x, sy); q.ib11 = __fdiv_rn(a2y, sy);
  const float ts = float(tile_size);
  const int max_tx = (Wp - 1) / tile_size, max_ty = (Hp - 1) / tile_size;
  int min_tx = int(floorf(__fdiv_rn(lox, ts))), min_ty = int(floorf(__fdiv_rn(loy, ts)));
  min_tx = max(min_tx, 0); min_ty = max(min_ty, 0);
  int hi_tx = int(ceilf(__fdiv_rn(hix, ts))), hi_ty = int(ceilf(__fdiv_rn(hiy, ts)));
  hi_tx = min(max(hi_tx, min_tx + 1), max_tx + 1);
  hi_ty = min(max(hi_ty, min_ty + 1), max_ty + 1);
  q.min_tx = min_tx; q.min_ty = min_ty;
  q.span_x = max(hi_tx - min_tx, 0); q.span_y = max(hi_ty - min_ty, 0);
  q.rel_min_x = float(min_tx * tile_size) - mx;
  q.rel_min_y = float(min_ty * tile_size) - my;
  return q;
}

// taichi_lib/grid_query.py:30-43 (separates_bbox) / :58-61 (test_tile)
__device__ __forceinline__ bool test_tile(const GridQuery& q, int u, int v, int tile_size) {
  const float lx = q.rel_min_x + float(u * tile_size), ly = q.rel_min_y + float(v * tile_size);
  const float ux = lx + float(tile_size), uy = ly + float(tile_size);
  {
    const float t0 = q.ib00 * lx + q.ib01 * ly, t1 = q.ib00 * ux + q.ib01 * ly;
    const float t2 = q.ib00 * ux + q.ib01 * uy, t3 = q.ib00 * lx + q.ib01 * uy;
    const float mn = fminf(fminf(t0, t1), fminf(t2, t3)), mxv = fmaxf(fmaxf(t0, t1), fmaxf(t2, t3));
    if (mn > 1.0f || mxv < -1.0f) return false;
  }
  {
    const float t0 = q.ib10 * lx + q.ib11 * ly, t1 = q.ib10 * ux + q.ib11 * ly;
    const float t2 = q.ib10 * ux + q.ib11 * uy, t3 = q.ib10 * lx + q.ib11 * uy;
    const float mn = fminf(fminf(t0, t1), fminf(t2, t3)), mxv = fmaxf(fmaxf(t0, t1), fmaxf(t2, t3));
    if (mn > 1.0f || mxv < -1.0f) return false;
  }
  return true;
}

// mapper/tile_mapper.py:34-40 (32-bit depth) / :53-59 (16-bit depth): the depth part only
__device__ __forceinline__ uint32_t depth_key(float depth, bool depth16) {
  if (!depth16) return gs_f32_bits(depth);
  const float d = depth < 0.f ? 0.f : (depth > 1.f ? 1.f : depth);
  return uint32_t(d * 65535.0f);
}

struct MapArgs {
  const float* points;
  const float* depth;
  int64_t v;            // number of Gaussians, or the buffer capacity when v_dev is set
  const int* v_dev;     // optional: the actual count lives on the device (no host read-back)
  int Wp, Hp, tile_size, tiles_wide;
  float thr;
  int depth16;
  GsShard sh;           // owned tile rows (the whole image when the call is not sharded)
};

// local tile id of an owned tile
__device__ __forceinline__ int local_tile(const MapArgs& a, int gx, int gy) {
  return gs_shard_local_row(a.sh, gy) * a.tiles_wide + gx;
}

__device__ __forceinline__ int64_t live_count(const MapArgs& a) {
  if (a.v_dev == nullptr) return a.v;
  const int64_t d = *a.v_dev;
  return d < a.v ? d : a.v;
}

// inclusive scan over the wave: row_shr 1/2/4/8 inside each 16-lane row, then row_bcast:15 / :31 across rows
__device__ __forceinline__ int wave_inclusive_scan(int x) {
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);
  return x;
}

// exclusive prefix of x over the 1024 threads of the workgroup (s_wave: 16 ints of LDS); total -> sum
__device__ __forceinline__ int block_exclusive_scan(int x, int* s_wave, int& sum) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int inc = wave_inclusive_scan(x);
  if (lane == 63) s_wave[wv] = inc;
  __syncthreads();
  int before = 0;
  sum = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    const int tot = s_wave[w];
    sum += tot;
    before += w < wv ? tot : 0;
  }
  __syncthreads();  // s_wave is reused by the caller's next round
  return before + inc - x;
}

// exclusive scan of row[0 .. n) in place by one workgroup of 1024 threads, in rounds of 1024 with a carry; returns the
// total (in every thread)
__device__ __forceinline__ int block_scan_row_in_place(int* row, int n, int* s_wave) {
  int carry = 0;
  for (int base = 0; base < n; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < n ? row[i] : 0;
    int total;
    const int before = block_exclusive_scan(v, s_wave, total);
    if (i < n) row[i] = carry + before;
    carry += total;
  }
  return carry;
}

inline int fill_args(MapArgs& a, int64_t v, const float* points, const float* depth, int width, int height,
                     const GsRasterConfig* cfg, int depth16, const GsRowShard* shard = nullptr) {
  if (int rc = gs_check_cfg(cfg)) return rc;
  GS_REQUIRE(width > 0 && height > 0, GS_ERR_INVALID_ARGUMENT, "mapper: image size %dx%d", width, height);
  GS_REQUIRE(v >= 0 && v < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT, "mapper: %lld gaussians", (long long)v);
  const int ts = cfg->tile_size;
  a.points = points; a.depth = depth; a.v = v; a.v_dev = nullptr;
  a.Wp = int(gs_div_up(width, ts)) * ts;  // pad_to_tile, tile_mapper.py:18-22
  a.Hp = int(gs_div_up(height, ts)) * ts;
  a.tile_size = ts;
  a.tiles_wide = a.Wp / ts;
  a.thr = cfg->alpha_threshold;
  a.depth16 = depth16;
  return gs_make_shard(shard, a.Hp / ts, &a.sh);
}

}  // namespace
