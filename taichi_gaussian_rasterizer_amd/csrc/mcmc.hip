// mcmc.hip -- the fixed-budget MCMC strategy ("3D Gaussian Splatting as Markov Chain Monte Carlo") on the device:
//   sample_rows        weighted draws with replacement, exact: weights quantised to 24-bit integers, an inclusive
//                      uint64 prefix (three-pass workgroup scan: sums per 2048 rows, one workgroup over the sums, the
//                      rows again), a binary search per draw, integer atomics for the copy counts
//   relocation_values  the opacity / scale correction of a row drawn `copies` times, evaluated in float64
//   apply              the corrected values written to a source and to all its copies
//   relocate_rows      the in-place row copy / zero fill of up to 32 tables by select mask, src_of and copy counts
//   perturb            position += R S^2 R^T (noise * gate(opacity) * scale), one launch over all rows; rows whose gate
//                      is zero cost their 4 bytes of alpha_logit and nothing else
// The library has no random numbers: the draws' 32-bit words and the noise are arguments.

#include "gs_common.h"

namespace {

constexpr int kThreads = 256;

// -------------------------------------------------------------------------------------------------------- sampling
constexpr int kRowsPerThread = 8;
constexpr int kRowsPerBlock = kThreads * kRowsPerThread;  // 2048
constexpr int kSumsThreads = 1024;

struct SampleArgs {
  int64_t n;
  const float* weights;
  const uint8_t* exclude;
};

// q = floor(clamp(w, 0, 1) * 2^24): NaN and negative weights give 0; the product with a power of two is exact
__device__ __forceinline__ uint32_t quantise(float w) {
  if (!(w > 0.0f)) return 0u;
  return w >= 1.0f ? (1u << 24) : uint32_t(w * 16777216.0f);
}

// the quantised weights of rows [i0, i0 + 8); rows at or behind n and excluded rows give 0.  i0 is a multiple of 8.
__device__ __forceinline__ void load_q8(const SampleArgs& a, int64_t i0, uint32_t (&q)[kRowsPerThread]) {
  float w[kRowsPerThread];
  if (i0 + kRowsPerThread <= a.n && (reinterpret_cast<uintptr_t>(a.weights) & 15) == 0) {
    const float4 lo = *reinterpret_cast<const float4*>(a.weights + i0);
    const float4 hi = *reinterpret_cast<const float4*>(a.weights + i0 + 4);
    w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w;
    w[4] = hi.x; w[5] = hi.y; w[6] = hi.z; w[7] = hi.w;
  } else {
#pragma unroll
    for (int e = 0; e < kRowsPerThread; ++e) w[e] = i0 + e < a.n ? a.weights[i0 + e] : 0.0f;
  }
#pragma unroll
  for (int e = 0; e < kRowsPerThread; ++e) {
    const bool out = a.exclude && i0 + e < a.n && a.exclude[i0 + e] != 0;
    q[e] = out ? 0u : quantise(w[e]);
  }
}

// inclusive prefix of `mine` over the workgroup (THREADS / 64 waves; s_wave: one word per wave) and the workgroup's
// total.  Two barriers: the caller may call it again with the same s_wave.
template <int THREADS>
__device__ __forceinline__ uint64_t block_inclusive_u64(uint64_t mine, uint64_t* s_wave, uint64_t& total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint64_t incl = mine;
#pragma unroll
  for (int off = 1; off < GS_WAVE; off <<= 1) {
    const uint64_t up = __shfl_up(incl, off);
    if (lane >= off) incl += up;
  }
  if (lane == GS_WAVE - 1) s_wave[wave] = incl;
  __syncthreads();
  total = 0;
#pragma unroll
  for (int w = 0; w < THREADS / GS_WAVE; ++w) {
    incl += w < wave ? s_wave[w] : 0;
    total += s_wave[w];
  }
  __syncthreads();
  return incl;
}

// pass 1: sums[b] = the quantised weights of workgroup b's 2048 rows
__global__ __launch_bounds__(kThreads) void sample_sums_kernel(SampleArgs a, uint64_t* sums) {
  __shared__ uint64_t s_wave[kThreads / GS_WAVE];
  const int64_t i0 = (int64_t(blockIdx.x) * kThreads + threadIdx.x) * kRowsPerThread;
  uint32_t q[kRowsPerThread];
  load_q8(a, i0, q);
  uint32_t mine = 0;  // 8 * 2^24 fits
#pragma unroll
  for (int e = 0; e < kRowsPerThread; ++e) mine += q[e];
  uint64_t total;
  block_inclusive_u64<kThreads>(mine, s_wave, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// pass 2: sums -> their exclusive prefix in place, sums[nb] = the total.  One workgroup walks the nb words in chunks of
// 1024 with a carry, so there is no limit on nb (2^20 for n just below 2^31: 1024 chunks).
__global__ __launch_bounds__(kSumsThreads) void sample_scan_sums_kernel(int nb, uint64_t* sums) {
  __shared__ uint64_t s_wave[kSumsThreads / GS_WAVE];
  uint64_t carry = 0;
  for (int base = 0; base < nb; base += kSumsThreads) {
    const int i = base + int(threadIdx.x);
    const uint64_t mine = i < nb ? sums[i] : 0;
    uint64_t total;
    const uint64_t incl = block_inclusive_u64<kSumsThreads>(mine, s_wave, total);
    if (i < nb) sums[i] = carry + incl - mine;
    carry += total;
  }
  if (threadIdx.x == 0) sums[nb] = carry;
}

// pass 3: cum[i] = the inclusive prefix of q, copies[i] = 0
__global__ __launch_bounds__(kThreads) void sample_cum_kernel(SampleArgs a, const uint64_t* sums, uint64_t* cum,
                                                              int32_t* copies) {
  __shared__ uint64_t s_wave[kThreads / GS_WAVE];
  const int64_t i0 = (int64_t(blockIdx.x) * kThreads + threadIdx.x) * kRowsPerThread;
  uint32_t q[kRowsPerThread];
  load_q8(a, i0, q);
  uint32_t mine = 0;
#pragma unroll
  for (int e = 0; e < kRowsPerThread; ++e) mine += q[e];
  uint64_t total;
  uint64_t run = sums[blockIdx.x] + block_inclusive_u64<kThreads>(mine, s_wave, total) - mine;
#pragma unroll
  for (int e = 0; e < kRowsPerThread; ++e) {
    run += q[e];
    if (i0 + e < a.n) {
      cum[i0 + e] = run;
      if (copies) copies[i0 + e] = 0;
    }
  }
}

struct DrawArgs {
  int64_t n, m;
  const uint64_t* cum;
  const uint64_t* total;  // one word: cum[n - 1]
  const uint32_t* random;
  const uint8_t* select;
  int32_t* out;
  int32_t* copies;
};

// draw j: t = floor(r * total / 2^32) < total, row = the first i with cum[i] > t (so q_i > 0)
__global__ __launch_bounds__(kThreads) void sample_draw_kernel(DrawArgs a) {
  const int64_t j = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (j >= a.m) return;
  const uint64_t total = *a.total;
  if ((a.select && a.select[j] == 0) || total == 0) {
    a.out[j] = int32_t(j);
    return;
  }
  const uint64_t t = __umul64hi(uint64_t(a.random[j]) << 32, total);
  int64_t lo = 0, hi = a.n - 1;  // cum[n - 1] = total > t: the answer lies in [lo, hi]
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a.cum[mid] > t) hi = mid;
    else lo = mid + 1;
  }
  a.out[j] = int32_t(lo);
  if (a.copies) atomicAdd(a.copies + lo, 1);
}

int64_t sample_blocks(int64_t n) { return gs_div_up(n, kRowsPerBlock); }
int64_t sample_cum_bytes(int64_t n) { return gs_align_up(n * 8, 256); }
int64_t sample_sums_bytes(int64_t n) { return gs_align_up((sample_blocks(n) + 1) * 8, 256); }

// ------------------------------------------------------------------------------------------------------ correction
struct ValuesArgs {
  int64_t n;
  const float* opacity;
  const float* log_scaling;
  const int32_t* copies;
  double min_opacity;
  float* new_alpha_logit;
  float* new_log_scaling;
};

// One lane per row; lanes of rows that were not drawn leave at once.  Everything between the float32 inputs and the
// float32 outputs is float64.  The binomial runs as a recurrence c <- c (i - 1 - k) / (k + 1) whose products stay
// below C(50, 25) * 25 < 2^53 and whose quotients are integers: exact.
__global__ __launch_bounds__(kThreads) void relocation_values_kernel(ValuesArgs a) {
  const int64_t row = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (row >= a.n) return;
  const int32_t drawn = a.copies[row];
  if (drawn <= 0) return;
  const int n = drawn >= GS_MCMC_N_MAX ? GS_MCMC_N_MAX : drawn + 1;
  const double o = double(a.opacity[row]);
  // 1 - (1 - o)^(1 / n) without the cancellation at small o; o = 1 gives 1, which the clamp takes back
  double x = -expm1(log1p(-o) / double(n));
  const double top = 1.0 - 1.1920928955078125e-07;  // 1 - 2^-23
  x = x < a.min_opacity ? a.min_opacity : x;
  x = x > top ? top : x;
  double denom = 0.0;
  for (int i = 1; i <= n; ++i) {
    double c = 1.0, p = x, sign = 1.0;
    for (int k = 0; k < i; ++k) {
      denom += sign * c * p / sqrt(double(k + 1));
      c = c * double(i - 1 - k) / double(k + 1);
      p *= x;
      sign = -sign;
    }
  }
  a.new_alpha_logit[row] = float(log(x / (1.0 - x)));
  const float shift = float(log(o / denom));
#pragma unroll
  for (int k = 0; k < 3; ++k) a.new_log_scaling[3 * row + k] = a.log_scaling[3 * row + k] + shift;
}

struct ApplyArgs {
  int64_t rows;
  const int32_t* src_of;
  const int32_t* copies;
  const float* new_alpha_logit;
  const float* new_log_scaling;
  float* out_alpha_logit;
  float* out_log_scaling;
};

__global__ __launch_bounds__(kThreads) void apply_kernel(ApplyArgs a) {
  const int64_t j = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (j >= a.rows) return;
  const int64_t s = a.src_of[j];
  if (a.copies[s] <= 0) return;
  a.out_alpha_logit[j] = a.new_alpha_logit[s];
#pragma unroll
  for (int k = 0; k < 3; ++k) a.out_log_scaling[3 * j + k] = a.new_log_scaling[3 * s + k];
}

// ------------------------------------------------------------------------------------------------- in-place tables
// The unit walk of move_rows_kernel (densify.hip): blockIdx.y = the column, 16-byte units where the row size and the
// pointer allow it, 4-byte units otherwise.  Only the few selected / drawn rows are read or written; every unit reads
// its row's select byte or copy count, which neighbouring lanes share.
constexpr int kRelocateMaxBlocks = 2048;

struct RelocateArgs {
  int64_t n;
  const int32_t* src_of;
  const uint8_t* select;
  const int32_t* copies;
  GsRelocateColumn col[GS_MOVE_COLUMNS_MAX];
};

template <typename Unit>
__device__ __forceinline__ void relocate_units(const GsRelocateColumn& c, const RelocateArgs& a) {
  const uint32_t per_row = uint32_t(c.row_bytes) / uint32_t(sizeof(Unit));
  const uint32_t total = uint32_t(a.n) * per_row;
  Unit* data = static_cast<Unit*>(c.data);
  const uint32_t step = gridDim.x * kThreads;
  // u + step stays below 2^32: the host checks total + step
  for (uint32_t u = blockIdx.x * kThreads + threadIdx.x; u < total; u += step) {
    const uint32_t j = u / per_row;
    if (c.mode == GS_RELOCATE_COPY) {
      // a selected row is never a source: no row is both read and written
      if (a.select[j] != 0) data[u] = data[int64_t(a.src_of[j]) * per_row + (u - j * per_row)];
    } else {
      // a selected row that drew nothing (no drawable row: src_of[j] == j) stays as it is
      const bool moved = c.mode == GS_RELOCATE_ZERO && a.select[j] != 0 && uint32_t(a.src_of[j]) != j;
      if (moved || a.copies[j] > 0) data[u] = Unit{};
    }
  }
}

__global__ __launch_bounds__(kThreads) void relocate_rows_kernel(RelocateArgs a) {
  const GsRelocateColumn& c = a.col[blockIdx.y];
  const bool wide = ((reinterpret_cast<uintptr_t>(c.data) | uintptr_t(c.row_bytes)) & 15) == 0;
  if (wide) relocate_units<uint4>(c, a);
  else relocate_units<uint32_t>(c, a);
}

// --------------------------------------------------------------------------------------------------------- perturb
struct PerturbArgs {
  int64_t n;
  float* position;
  const float* log_scaling;
  const float* rotation;
  const float* alpha_logit;
  const float* noise;
  float scale, k, x0;
};

// One lane per row.  The gate comes from the row's 4 bytes of alpha_logit; where it is exactly zero (expf overflows from
// k ((1 - o) - x0) < -88.7 on: o > 0.89 with the defaults) the lane is done, and a wave of such rows issues nothing more.
// The other rows read 12 + 12 + 16 + 12 bytes and write their 12 bytes of position only where its bits change.
__global__ __launch_bounds__(kThreads) void perturb_kernel(PerturbArgs a) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= a.n) return;
  const float o = 1.0f / (1.0f + expf(-a.alpha_logit[i]));
  const float g = 1.0f / (1.0f + expf(-a.k * ((1.0f - o) - a.x0)));
  if (g == 0.0f) return;
  const float4 q = *reinterpret_cast<const float4*>(a.rotation + 4 * i);  // xyzw; the host checks the alignment
  const float qlen = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  const float x = q.x / qlen, y = q.y / qlen, z = q.z / qlen, w = q.w / qlen;
  const float gs = g * a.scale;
  float v[3], s2[3], p[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    v[k] = a.noise[3 * i + k] * gs;
    const float s = expf(a.log_scaling[3 * i + k]);
    s2[k] = s * s;
    p[k] = a.position[3 * i + k];
  }
  const float x2 = x * x, y2 = y * y, z2 = z * z;
  const float R[3][3] = {{1 - 2 * y2 - 2 * z2, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y},
                         {2 * x * y + 2 * w * z, 1 - 2 * x2 - 2 * z2, 2 * y * z - 2 * w * x},
                         {2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x2 - 2 * y2}};
  float t[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) t[c] = s2[c] * (R[0][c] * v[0] + R[1][c] * v[1] + R[2][c] * v[2]);  // S^2 R^T v
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float d = R[r][0] * t[0] + R[r][1] * t[1] + R[r][2] * t[2];
    // d == 0 keeps the bits (-0.0f + 0.0f would be +0.0f); a d below half an ulp of the position changes nothing either
    const float moved = d == 0.0f ? p[r] : p[r] + d;
    if (__float_as_uint(moved) != __float_as_uint(p[r])) a.position[3 * i + r] = moved;
  }
}

}  // namespace

extern "C" int64_t gs_sample_rows_scratch_bytes(int64_t n) {
  if (n <= 0) return 0;
  return sample_cum_bytes(n) + sample_sums_bytes(n);
}

extern "C" int gs_sample_rows(int64_t n, const float* weights, const uint8_t* exclude, int64_t m,
                              const uint32_t* random, const uint8_t* select, int32_t* out, int32_t* copies,
                              void* scratch, int64_t scratch_bytes, void* stream) {
  GS_REQUIRE(n >= 0 && n < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT,
             "gs_sample_rows: %lld rows (0 .. 2^31 - 1)", (long long)n);
  GS_REQUIRE(m >= 0 && m < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT,
             "gs_sample_rows: %lld draws (0 .. 2^31 - 1)", (long long)m);
  GS_REQUIRE(!select || m == n, GS_ERR_INVALID_ARGUMENT,
             "gs_sample_rows: a select mask needs one draw per row (%lld draws, %lld rows)", (long long)m,
             (long long)n);
  if (n == 0 && m == 0) return GS_OK;
  GS_REQUIRE(n > 0, GS_ERR_INVALID_ARGUMENT, "gs_sample_rows: %lld draws from an empty table", (long long)m);
  GS_REQUIRE(weights, GS_ERR_INVALID_ARGUMENT, "gs_sample_rows: NULL buffer (weights)");
  GS_REQUIRE(m == 0 || (random && out), GS_ERR_INVALID_ARGUMENT, "gs_sample_rows: NULL buffer (random or out)");
  GS_REQUIRE(scratch, GS_ERR_INVALID_ARGUMENT, "gs_sample_rows: NULL buffer (scratch)");
  GS_REQUIRE(scratch_bytes >= gs_sample_rows_scratch_bytes(n), GS_ERR_SCRATCH_TOO_SMALL,
             "gs_sample_rows: scratch of %lld bytes, %lld needed", (long long)scratch_bytes,
             (long long)gs_sample_rows_scratch_bytes(n));
  GS_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, GS_ERR_INVALID_ARGUMENT,
             "gs_sample_rows: scratch is not 16-byte aligned");
  GS_REQUIRE(((reinterpret_cast<uintptr_t>(weights) | reinterpret_cast<uintptr_t>(random) |
               reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(copies)) & 3) == 0,
             GS_ERR_INVALID_ARGUMENT, "gs_sample_rows: weights, random, out and copies must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nb = int(sample_blocks(n));
  const SampleArgs a{n, weights, exclude};
  uint64_t* cum = static_cast<uint64_t*>(scratch);
  uint64_t* sums = reinterpret_cast<uint64_t*>(static_cast<char*>(scratch) + sample_cum_bytes(n));
  hipLaunchKernelGGL(sample_sums_kernel, dim3(unsigned(nb)), dim3(kThreads), 0, s, a, sums);
  hipLaunchKernelGGL(sample_scan_sums_kernel, dim3(1), dim3(kSumsThreads), 0, s, nb, sums);
  hipLaunchKernelGGL(sample_cum_kernel, dim3(unsigned(nb)), dim3(kThreads), 0, s, a, sums, cum, copies);
  if (m > 0) {
    const DrawArgs d{n, m, cum, sums + nb, random, select, out, copies};
    hipLaunchKernelGGL(sample_draw_kernel, dim3(unsigned(gs_div_up(m, kThreads))), dim3(kThreads), 0, s, d);
  }
  GS_CHECK_LAUNCH("gs_sample_rows");
  return GS_OK;
}

extern "C" int gs_mcmc_relocation_values(int64_t n, const float* opacity, const float* log_scaling,
                                         const int32_t* copies, float min_opacity, float* new_alpha_logit,
                                         float* new_log_scaling, void* stream) {
  GS_REQUIRE(n >= 0 && n < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT,
             "gs_mcmc_relocation_values: %lld rows (0 .. 2^31 - 1)", (long long)n);
  GS_REQUIRE(min_opacity > 0.0f && min_opacity < 1.0f, GS_ERR_INVALID_ARGUMENT,
             "gs_mcmc_relocation_values: min_opacity %g not inside (0, 1)", double(min_opacity));
  if (n == 0) return GS_OK;
  GS_REQUIRE(opacity && log_scaling && copies && new_alpha_logit && new_log_scaling, GS_ERR_INVALID_ARGUMENT,
             "gs_mcmc_relocation_values: NULL buffer");
  const ValuesArgs a{n, opacity, log_scaling, copies, double(min_opacity), new_alpha_logit, new_log_scaling};
  hipLaunchKernelGGL(relocation_values_kernel, dim3(unsigned(gs_div_up(n, kThreads))), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), a);
  GS_CHECK_LAUNCH("gs_mcmc_relocation_values");
  return GS_OK;
}

extern "C" int gs_mcmc_apply(int64_t rows_out, const int32_t* src_of, const int32_t* copies,
                             const float* new_alpha_logit, const float* new_log_scaling, float* out_alpha_logit,
                             float* out_log_scaling, void* stream) {
  GS_REQUIRE(rows_out >= 0 && rows_out < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT,
             "gs_mcmc_apply: %lld rows (0 .. 2^31 - 1)", (long long)rows_out);
  if (rows_out == 0) return GS_OK;
  GS_REQUIRE(src_of && copies && new_alpha_logit && new_log_scaling && out_alpha_logit && out_log_scaling,
             GS_ERR_INVALID_ARGUMENT, "gs_mcmc_apply: NULL buffer");
  const ApplyArgs a{rows_out, src_of, copies, new_alpha_logit, new_log_scaling, out_alpha_logit, out_log_scaling};
  hipLaunchKernelGGL(apply_kernel, dim3(unsigned(gs_div_up(rows_out, kThreads))), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), a);
  GS_CHECK_LAUNCH("gs_mcmc_apply");
  return GS_OK;
}

extern "C" int gs_table_relocate_rows(int64_t n, const int32_t* src_of, const uint8_t* select, const int32_t* copies,
                                      int32_t columns, const GsRelocateColumn* columns_host, void* stream) {
  GS_REQUIRE(n >= 0 && n < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT, "gs_table_relocate_rows: %lld rows",
             (long long)n);
  GS_REQUIRE(columns >= 0 && columns <= GS_MOVE_COLUMNS_MAX, GS_ERR_INVALID_ARGUMENT,
             "gs_table_relocate_rows: columns %d not in [0,%d]", columns, GS_MOVE_COLUMNS_MAX);
  if (n == 0 || columns == 0) return GS_OK;
  GS_REQUIRE(columns_host, GS_ERR_INVALID_ARGUMENT, "gs_table_relocate_rows: NULL buffer (columns)");
  RelocateArgs a{};
  a.n = n;
  a.src_of = src_of;
  a.select = select;
  a.copies = copies;
  int64_t most_units = 0;
  bool selecting = false, counting = false;
  for (int k = 0; k < columns; ++k) {
    const GsRelocateColumn& c = columns_host[k];
    GS_REQUIRE(c.row_bytes >= 4 && c.row_bytes % 4 == 0, GS_ERR_INVALID_ARGUMENT,
               "gs_table_relocate_rows: column %d has rows of %d bytes (a positive multiple of 4)", k, c.row_bytes);
    GS_REQUIRE(c.mode == GS_RELOCATE_COPY || c.mode == GS_RELOCATE_ZERO || c.mode == GS_RELOCATE_ZERO_SOURCES,
               GS_ERR_INVALID_ARGUMENT, "gs_table_relocate_rows: column %d has mode %d", k, c.mode);
    GS_REQUIRE(c.data, GS_ERR_INVALID_ARGUMENT, "gs_table_relocate_rows: NULL buffer (column %d)", k);
    GS_REQUIRE((reinterpret_cast<uintptr_t>(c.data) & 3) == 0, GS_ERR_INVALID_ARGUMENT,
               "gs_table_relocate_rows: column %d is not 4-byte aligned", k);
    a.col[k] = c;
    const bool wide = ((reinterpret_cast<uintptr_t>(c.data) | uintptr_t(c.row_bytes)) & 15) == 0;
    const int64_t units = n * (c.row_bytes / (wide ? 16 : 4));
    most_units = units > most_units ? units : most_units;
    selecting = selecting || c.mode != GS_RELOCATE_ZERO_SOURCES;
    counting = counting || c.mode != GS_RELOCATE_COPY;
  }
  GS_REQUIRE(src_of || !selecting, GS_ERR_INVALID_ARGUMENT, "gs_table_relocate_rows: NULL buffer (src_of)");
  GS_REQUIRE(select || !selecting, GS_ERR_INVALID_ARGUMENT, "gs_table_relocate_rows: NULL buffer (select)");
  GS_REQUIRE(copies || !counting, GS_ERR_INVALID_ARGUMENT, "gs_table_relocate_rows: NULL buffer (copies)");
  const int64_t blocks = gs_div_up(most_units, kThreads);
  const unsigned grid_x = unsigned(blocks < kRelocateMaxBlocks ? blocks : kRelocateMaxBlocks);
  GS_REQUIRE(most_units + int64_t(grid_x) * kThreads < (int64_t(1) << 32), GS_ERR_UNSUPPORTED,
             "gs_table_relocate_rows: a column of %lld units of 4 or 16 bytes (below 2^32 less one grid stride)",
             (long long)most_units);
  hipLaunchKernelGGL(relocate_rows_kernel, dim3(grid_x, unsigned(columns)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), a);
  GS_CHECK_LAUNCH("gs_table_relocate_rows");
  return GS_OK;
}

extern "C" int gs_mcmc_perturb(int64_t n, float* position, const float* log_scaling, const float* rotation,
                               const float* alpha_logit, const float* noise, float scale, float k, float x0,
                               void* stream) {
  GS_REQUIRE(n >= 0 && n < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT, "gs_mcmc_perturb: %lld rows (0 .. 2^31 - 1)",
             (long long)n);
  if (n == 0) return GS_OK;
  GS_REQUIRE(position && log_scaling && rotation && alpha_logit && noise, GS_ERR_INVALID_ARGUMENT,
             "gs_mcmc_perturb: NULL buffer");
  GS_REQUIRE((reinterpret_cast<uintptr_t>(rotation) & 15) == 0, GS_ERR_INVALID_ARGUMENT,
             "gs_mcmc_perturb: rotation is not 16-byte aligned");
  const PerturbArgs a{n, position, log_scaling, rotation, alpha_logit, noise, scale, k, x0};
  hipLaunchKernelGGL(perturb_kernel, dim3(unsigned(gs_div_up(n, kThreads))), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), a);
  GS_CHECK_LAUNCH("gs_mcmc_perturb");
  return GS_OK;
}
