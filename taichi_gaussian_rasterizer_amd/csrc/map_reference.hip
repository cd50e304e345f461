// map_reference.hip -- the reference-shaped mapper primitives (gs_tile_count, gs_full_cumsum_i32, gs_tile_emit_keys,
// gs_find_ranges; gs_radix_sort_pairs lives in radix_sort.hip).  They run the reference's own stage sequence
// (mapper/tile_mapper.py:74-196) on the query of map_query.h and are used to cross-check the fused path of mapper.hip;
// gs_selftest_detmath exposes the deterministic square root and logarithm that query is built on.
//
// COMPILED WITH -ffp-contract=off (map_query.h).

#include "map_query.h"

namespace {

__global__ __launch_bounds__(256) void tile_count_kernel(MapArgs a, int* counts) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= live_count(a)) return;
  const GridQuery q = grid_query(a.points + 7 * i, a.Wp, a.Hp, a.tile_size, a.thr);
  int c = 0;
  for (int ty = 0; ty < q.span_y; ++ty)
    for (int tx = 0; tx < q.span_x; ++tx) c += test_tile(q, tx, ty, a.tile_size) ? 1 : 0;
  counts[i] = c;
}

__global__ __launch_bounds__(256) void tile_emit_keys_kernel(MapArgs a, const int* offsets, uint64_t* keys,
                                                             int* values) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= live_count(a)) return;
  const GridQuery q = grid_query(a.points + 7 * i, a.Wp, a.Hp, a.tile_size, a.thr);
  int64_t k = offsets[i];
  const uint64_t dk = depth_key(a.depth[i], a.depth16 != 0);
  const int shift = a.depth16 ? 16 : 32;
  // ti.ndrange(span.x, span.y): x outer, y inner (tile_mapper.py:134)
  for (int tx = 0; tx < q.span_x; ++tx)
    for (int ty = 0; ty < q.span_y; ++ty)
      if (test_tile(q, tx, ty, a.tile_size)) {
        const int tile_id = (tx + q.min_tx) + (ty + q.min_ty) * a.tiles_wide;
        keys[k] = dk | (uint64_t(uint32_t(tile_id)) << shift);
        values[k] = int(i);
        ++k;
      }
}

__global__ __launch_bounds__(256) void find_ranges_kernel(int64_t k, const uint64_t* keys, int shift, int* ranges) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int64_t t = int64_t(keys[i] >> shift);
  if (i == 0 || int64_t(keys[i - 1] >> shift) != t) ranges[2 * t] = int(i);
  if (i + 1 == k || int64_t(keys[i + 1] >> shift) != t) ranges[2 * t + 1] = int(i + 1);
}

// block-level exclusive scan, 3 kernels: (1) per-block sums, (2) scan of sums (one block),
// (3) per-block scan + offset.  1024 elements per block (256 threads x 4).
constexpr int SCAN_BLOCK = 1024;

__global__ __launch_bounds__(256) void scan_block_sums(int64_t n, const int* in, int* sums) {
  __shared__ int s[256];
  const int64_t base = int64_t(blockIdx.x) * SCAN_BLOCK;
  int acc = 0;
  for (int e = 0; e < 4; ++e) {
    const int64_t i = base + threadIdx.x * 4 + e;
    if (i < n) acc += in[i];
  }
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = s[0];
}

__global__ __launch_bounds__(1024) void scan_sums(int nb, int* sums) {  // exclusive, in place, single block
  __shared__ int s_wave[16];
  block_scan_row_in_place(sums, nb, s_wave);
}

__global__ __launch_bounds__(256) void scan_apply(int64_t n, const int* in, const int* sums, int* out) {
  __shared__ int s[256];
  const int64_t base = int64_t(blockIdx.x) * SCAN_BLOCK;
  int v[4], acc = 0;
  for (int e = 0; e < 4; ++e) {
    const int64_t i = base + threadIdx.x * 4 + e;
    v[e] = i < n ? in[i] : 0;
    acc += v[e];
  }
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    int x = s[threadIdx.x];
    if (threadIdx.x >= off) x += s[threadIdx.x - off];
    __syncthreads();
    s[threadIdx.x] = x;
    __syncthreads();
  }
  int run = sums[blockIdx.x] + s[threadIdx.x] - acc;
  for (int e = 0; e < 4; ++e) {
    const int64_t i = base + threadIdx.x * 4 + e;
    if (i < n) out[i] = run;
    run += v[e];
    if (i == n - 1) out[n] = run;  // the total, appended (full_cumsum.cu:36-41)
  }
}

__global__ __launch_bounds__(256) void detmath_kernel(int64_t n, const float* x, float* sqrt_out, float* log_out) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  if (sqrt_out) sqrt_out[i] = gs_det_sqrtf(x[i]);
  if (log_out) log_out[i] = gs_det_logf(x[i]);
}

}  // namespace

extern "C" int gs_selftest_detmath(int64_t n, const float* x, float* sqrt_out, float* log_out, void* stream) {
  if (n == 0) return GS_OK;
  GS_REQUIRE(x, GS_ERR_INVALID_ARGUMENT, "gs_selftest_detmath: x is NULL");
  hipLaunchKernelGGL(detmath_kernel, dim3(unsigned(gs_div_up(n, 256))), dim3(256), 0, static_cast<hipStream_t>(stream),
                     n, x, sqrt_out, log_out);
  GS_CHECK_LAUNCH("gs_selftest_detmath");
  return GS_OK;
}

extern "C" int gs_tile_count(int64_t v, const float* points, int32_t width, int32_t height,
                             const GsRasterConfig* cfg, int32_t* counts, void* stream) {
  MapArgs a;
  if (int rc = fill_args(a, v, points, nullptr, width, height, cfg, 0)) return rc;
  if (v == 0) return GS_OK;
  GS_REQUIRE(points && counts, GS_ERR_INVALID_ARGUMENT, "gs_tile_count: NULL buffer");
  hipLaunchKernelGGL(tile_count_kernel, dim3(unsigned(gs_div_up(v, 256))), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a, counts);
  GS_CHECK_LAUNCH("gs_tile_count");
  return GS_OK;
}

extern "C" int64_t gs_cumsum_scratch_bytes(int64_t n) { return gs_align_up((gs_div_up(n, SCAN_BLOCK) + 1) * 4, 256); }

extern "C" int gs_full_cumsum_i32(int64_t n, const int32_t* in, int32_t* out, void* scratch, int64_t scratch_bytes,
                                  void* stream) {
  GS_REQUIRE(n >= 0 && out, GS_ERR_INVALID_ARGUMENT, "gs_full_cumsum_i32: bad arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) return gs_memset_async(out, 4, s, "gs_full_cumsum_i32: memset failed");
  GS_REQUIRE(in && scratch && scratch_bytes >= gs_cumsum_scratch_bytes(n), GS_ERR_SCRATCH_TOO_SMALL,
             "gs_full_cumsum_i32: scratch %lld < %lld", (long long)scratch_bytes, (long long)gs_cumsum_scratch_bytes(n));
  const int nb = int(gs_div_up(n, SCAN_BLOCK));
  int* sums = static_cast<int*>(scratch);
  hipLaunchKernelGGL(scan_block_sums, dim3(nb), dim3(256), 0, s, n, in, sums);
  hipLaunchKernelGGL(scan_sums, dim3(1), dim3(1024), 0, s, nb, sums);
  hipLaunchKernelGGL(scan_apply, dim3(nb), dim3(256), 0, s, n, in, sums, out);
  GS_CHECK_LAUNCH("gs_full_cumsum_i32");
  return GS_OK;
}

extern "C" int gs_tile_emit_keys(int64_t v, const float* points, const float* depth, const int32_t* offsets,
                                 int32_t width, int32_t height, const GsRasterConfig* cfg, int32_t use_depth16,
                                 uint64_t* keys, int32_t* values, void* stream) {
  MapArgs a;
  if (int rc = fill_args(a, v, points, depth, width, height, cfg, use_depth16)) return rc;
  if (v == 0) return GS_OK;
  GS_REQUIRE(points && depth && offsets && keys && values, GS_ERR_INVALID_ARGUMENT, "gs_tile_emit_keys: NULL buffer");
  hipLaunchKernelGGL(tile_emit_keys_kernel, dim3(unsigned(gs_div_up(v, 256))), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a, offsets, keys, values);
  GS_CHECK_LAUNCH("gs_tile_emit_keys");
  return GS_OK;
}

extern "C" int gs_find_ranges(int64_t k, const uint64_t* sorted_keys, int32_t use_depth16, int64_t num_tiles,
                              int32_t* tile_ranges, void* stream) {
  GS_REQUIRE(tile_ranges && num_tiles > 0, GS_ERR_INVALID_ARGUMENT, "gs_find_ranges: bad arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = gs_memset_async(tile_ranges, size_t(num_tiles) * 8, s, "gs_find_ranges: memset failed")) return rc;
  if (k == 0) return GS_OK;
  GS_REQUIRE(sorted_keys, GS_ERR_INVALID_ARGUMENT, "gs_find_ranges: keys is NULL");
  hipLaunchKernelGGL(find_ranges_kernel, dim3(unsigned(gs_div_up(k, 256))), dim3(256), 0, s, k, sorted_keys,
                     use_depth16 ? 16 : 32, tile_ranges);
  GS_CHECK_LAUNCH("gs_find_ranges");
  return GS_OK;
}
