// f64_common.h -- shared by the float64 translation units (project_f64.hip, sh_f64.hip, raster_f64.hip).
//
// Determinism: gradcheck runs a backward twice and requires identical bits, so no float atomic feeds a result.  Sums
// over the entries of one Gaussian (SH list entries, rasterizer (tile, entry) records) run in ascending entry order:
// gs_f64_group sorts the (key, entry) pairs stably and gives every key its run of entries.
#pragma once
#include "gs_common.h"

// Every lane ends with the wave's sum; lane 0's value is what callers keep.  The butterfly order is fixed, so the
// result is the same bits on every run.
__device__ __forceinline__ double gs_f64_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// Sum of `x` over a workgroup of NW waves, in a fixed order (waves in order after the butterfly).  `s` holds NW
// doubles; every thread returns the total.  Contains two barriers: call it from every thread.
template <int NW>
__device__ __forceinline__ double gs_f64_block_sum(double x, double* s) {
  x = gs_f64_wave_sum(x);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = x;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < NW; ++w) t += s[w];
  __syncthreads();
  return t;
}

// Entries grouped by key: keys (k) are uint32 (key_bytes 4) or uint64 (key_bytes 8) in [0, n).  On return
// order[seg[2 j] .. seg[2 j + 1]) are the entries whose key is j, ascending; keys with no entry have an empty run.
// Keys outside [0, n) belong to no run.
int64_t gs_f64_group_scratch_bytes(int64_t k, int64_t n, int key_bytes);
int gs_f64_group(int64_t k, int key_bytes, const void* keys, int64_t n, int32_t** order, int32_t** seg, void* scratch,
                 int64_t scratch_bytes, hipStream_t stream);
