// knn.hip -- exact k nearest neighbours of every point of a 3D point cloud (the simple-knn step that gives a new
// Gaussian its first scale), reshaped for wave64.
//   bbox     partial boxes of the finite points, one per workgroup (every later kernel folds the <= 256 partials itself)
//   codes    48-bit Morton code (16 bits per axis) of every point normalised to the box, + the identity permutation
//   sort     gs_radix_sort_pairs on the codes: spatially close points become close in the order
//   gather   packed 16-byte records (x, y, z, bits of the original index) in sorted order, padded with NaN records to a
//            whole number of RUNS of 256, and one box per run
//   query    one workgroup per run, one lane per query, the best k (d2, j) pairs in registers.  The list is seeded from
//            the own run; every wave then walks the other runs outwards from its own and skips a run when the box of the
//            wave's 64 queries is further from the run's box than the wave's largest k-th distance.
//
// EXACTNESS.  d2(i, j) is the float32 value of (dx * dx + dy * dy) + dz * dz with d = p_j - p_i, in this order and
// without contraction (the unit is compiled with -ffp-contract=off), and a row lists the k smallest (d2, j) pairs in
// lexicographic order.  A run is skipped only by a lower bound of the d2 of every pair it could contribute: per axis
// the gap g between two boxes (or a point and a box) is one float32 subtraction of two coordinates that bracket the
// true difference, c - p >= lo_c - hi_p > 0 in exact arithmetic, and rounding is monotone, so |fl(c - p)| >= fl(g);
// the squares, the two sums and their roundings are monotone as well, so the bound put through the SAME operation
// order never exceeds the d2 the scan would compute.  Skips test `bound > k-th distance` strictly: a candidate at
// exactly the k-th distance with a smaller index is still seen.  The order of the walk and the quality of the codes
// change the speed only.
//
// A point with a non-finite coordinate is stored as a NaN record: no `d2 < worst` or `d2 == worst` test accepts it, the
// boxes (fminf / fmaxf) ignore it, and as a query it scans nothing, so its row stays +inf / -1.

#include <limits.h>
#include <math.h>

#include "gs_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kRun = 256;             // records per run = queries per workgroup
constexpr int kWaves = kThreads / GS_WAVE;
constexpr int kMaxPartials = 256;     // workgroups of the box reduction
constexpr int kCodeBits = 16;         // per axis
constexpr int kNoIndex = INT_MAX;     // list entries that hold no neighbour (n < 2^31, so no row has this index)

struct Box {
  float lo[3], hi[3];
};

__device__ __forceinline__ Box empty_box() {
  return Box{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
}
__device__ __forceinline__ void box_add(Box& b, float x, float y, float z) {  // fminf / fmaxf drop a NaN operand
  b.lo[0] = fminf(b.lo[0], x); b.lo[1] = fminf(b.lo[1], y); b.lo[2] = fminf(b.lo[2], z);
  b.hi[0] = fmaxf(b.hi[0], x); b.hi[1] = fmaxf(b.hi[1], y); b.hi[2] = fmaxf(b.hi[2], z);
}
__device__ __forceinline__ Box wave_box(Box b) {  // every lane gets the box of the wave
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      b.lo[a] = fminf(b.lo[a], __shfl_xor(b.lo[a], off));
      b.hi[a] = fmaxf(b.hi[a], __shfl_xor(b.hi[a], off));
    }
  return b;
}
// the box of the workgroup in every thread (one barrier; s_box: 6 floats per wave)
__device__ __forceinline__ Box block_box(Box b, float (*s_box)[6]) {
  b = wave_box(b);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s_box[wave][a] = b.lo[a];
      s_box[wave][3 + a] = b.hi[a];
    }
  __syncthreads();
  Box r = empty_box();
#pragma unroll
  for (int w = 0; w < kWaves; ++w)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      r.lo[a] = fminf(r.lo[a], s_box[w][a]);
      r.hi[a] = fmaxf(r.hi[a], s_box[w][3 + a]);
    }
  return r;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;  // false for NaN
}

// ------------------------------------------------------------------------------------------------------- bbox, codes
// partials (kMaxPartials, 8): lo xyz, hi xyz of the finite points of one workgroup's stride; gridDim.x partials
__global__ __launch_bounds__(kThreads) void knn_bbox_kernel(int64_t n, const float* __restrict__ points,
                                                            float* __restrict__ partials) {
  __shared__ float s_box[kWaves][6];
  Box b = empty_box();
  const int64_t step = int64_t(gridDim.x) * kThreads;
  for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += step) {
    const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
    if (finite3(x, y, z)) box_add(b, x, y, z);
  }
  b = block_box(b, s_box);
  if (threadIdx.x == 0) {
    float* out = partials + 8 * blockIdx.x;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      out[a] = b.lo[a];
      out[4 + a] = b.hi[a];
    }
  }
}

__device__ __forceinline__ uint64_t spread16(uint64_t x) {  // bit i -> bit 3 i, 16 bits
  x &= 0xffffull;
  x = (x | (x << 16)) & 0x0000ff0000ffull;
  x = (x | (x << 8)) & 0x00f00f00f00full;
  x = (x | (x << 4)) & 0x0c30c30c30c3ull;
  x = (x | (x << 2)) & 0x249249249249ull;
  return x;
}

// cell of p on an axis [lo, hi] of the box.  An axis without extent (a line, a plane, one point, no finite point at
// all) has cell 0; a quotient that is NaN (an extent that overflowed to inf) falls to 0 in fmaxf.
__device__ __forceinline__ uint32_t axis_cell(float p, float lo, float hi) {
  const float extent = hi - lo;
  if (!(extent > 0.0f)) return 0u;
  const float top = float((1 << kCodeBits) - 1);
  return uint32_t(fminf(fmaxf((p - lo) / extent * top, 0.0f), top));
}

__global__ __launch_bounds__(kThreads) void knn_codes_kernel(int64_t n, const float* __restrict__ points,
                                                             const float* __restrict__ partials, int num_partials,
                                                             uint64_t* __restrict__ codes, int32_t* __restrict__ order) {
  __shared__ float s_box[kWaves][6];
  Box b = empty_box();
  if (int(threadIdx.x) < num_partials) {  // num_partials <= kMaxPartials = kThreads
    const float* p = partials + 8 * threadIdx.x;
    b = Box{{p[0], p[1], p[2]}, {p[4], p[5], p[6]}};
  }
  b = block_box(b, s_box);
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= n) return;
  const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
  uint64_t code = (uint64_t(1) << (3 * kCodeBits)) - 1;  // the non-finite points sort to the end
  if (finite3(x, y, z))
    code = spread16(axis_cell(x, b.lo[0], b.hi[0])) | (spread16(axis_cell(y, b.lo[1], b.hi[1])) << 1) |
           (spread16(axis_cell(z, b.lo[2], b.hi[2])) << 2);
  codes[i] = code;
  order[i] = int32_t(i);
}

// ------------------------------------------------------------------------------------------------------------ gather
// records (runs * 256) float4, boxes (runs, 8): lo xyz, hi xyz of the run's finite records
__global__ __launch_bounds__(kThreads) void knn_gather_kernel(int64_t n, const float* __restrict__ points,
                                                              const int32_t* __restrict__ order,
                                                              float4* __restrict__ records, float* __restrict__ boxes) {
  __shared__ float s_box[kWaves][6];
  const int64_t s = int64_t(blockIdx.x) * kRun + threadIdx.x;
  float4 rec = make_float4(NAN, NAN, NAN, __int_as_float(-1));
  if (s < n) {
    const int32_t i = order[s];
    const float x = points[3 * int64_t(i)], y = points[3 * int64_t(i) + 1], z = points[3 * int64_t(i) + 2];
    rec.w = __int_as_float(i);
    if (finite3(x, y, z)) { rec.x = x; rec.y = y; rec.z = z; }
  }
  records[s] = rec;  // s < runs * 256: the buffer is padded to whole runs
  Box b = empty_box();
  box_add(b, rec.x, rec.y, rec.z);
  b = block_box(b, s_box);
  if (threadIdx.x == 0) {
    float* out = boxes + 8 * int64_t(blockIdx.x);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      out[a] = b.lo[a];
      out[4 + a] = b.hi[a];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- query
// THE distance: this operation order is the contract (see the head of the file)
__device__ __forceinline__ float dist2(float dx, float dy, float dz) { return (dx * dx + dy * dy) + dz * dz; }

// lower bound of dist2 between any point of [qlo, qhi] and any point of [clo, chi], through the same operations.
// Empty boxes (lo = +inf, hi = -inf) give +inf, never NaN: no operand pair is (inf, inf) of one sign.
__device__ __forceinline__ float box_gap(float qlo, float qhi, float clo, float chi) {
  return fmaxf(0.0f, fmaxf(clo - qhi, qlo - chi));
}
__device__ __forceinline__ float box_dist2(const Box& q, const float* __restrict__ c) {
  return dist2(box_gap(q.lo[0], q.hi[0], c[0], c[4]), box_gap(q.lo[1], q.hi[1], c[1], c[5]),
               box_gap(q.lo[2], q.hi[2], c[2], c[6]));
}

__device__ __forceinline__ bool pair_less(float d, int j, float od, int oj) { return d < od || (d == od && j < oj); }

// The best-k list: (d[i], j[i]) ascending for i < k, entries from k on unused.  CAP is the register capacity; every
// index is a compile-time constant after unrolling and `i < k` is wave-uniform.  (wd, wj) = entry k - 1.
template <int CAP>
struct BestK {
  float d[CAP];
  int j[CAP];
  float wd;
  int wj;

  __device__ __forceinline__ void init() {
#pragma unroll
    for (int i = 0; i < CAP; ++i) {
      d[i] = INFINITY;
      j[i] = kNoIndex;
    }
    wd = INFINITY;
    wj = kNoIndex;
  }

  // a NaN distance fails both comparisons
  __device__ __forceinline__ void offer(int k, float cd, int cj) {
    if (!pair_less(cd, cj, wd, wj)) return;
    bool placed = false;  // the old entry k - 1 drops out; entries move down until the candidate's place is free
#pragma unroll
    for (int i = CAP - 1; i >= 0; --i) {
      if (i < k) {
        const int below = i > 0 ? i - 1 : 0;
        const bool up = i > 0 && pair_less(cd, cj, d[below], j[below]);
        const float nd = up ? d[below] : cd;
        const int nj = up ? j[below] : cj;
        d[i] = placed ? d[i] : nd;
        j[i] = placed ? j[i] : nj;
        placed = placed || !up;
      }
    }
#pragma unroll
    for (int i = 0; i < CAP; ++i)
      if (i == k - 1) {
        wd = d[i];
        wj = j[i];
      }
  }

  // all 256 records of a staged run; every lane reads the same address (an LDS broadcast)
  __device__ __forceinline__ void scan(int k, const float4* s_rec, const float4& me, int my_index) {
#pragma unroll 4
    for (int c = 0; c < kRun; ++c) {
      const float4 r = s_rec[c];
      const int cj = __float_as_int(r.w);
      const float cd = dist2(r.x - me.x, r.y - me.y, r.z - me.z);
      if (cj != my_index) offer(k, cd, cj);  // the point itself is excluded by index: a duplicate is a neighbour
    }
  }
};

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off));
  return x;
}

// LDS: the own run (4 KiB) and one 4 KiB staging buffer per wave, 20 KiB per workgroup.  A wave stages and scans on
// its own, so the walk needs no workgroup barrier and the skip decision stays per wave.  Staging writes 16 bytes per
// lane at consecutive addresses (conflict-free); the scan reads one address per instruction (broadcast).
template <int CAP>
__global__ __launch_bounds__(kThreads) void knn_query_kernel(int64_t n, int runs, int k,
                                                             const float4* __restrict__ records,
                                                             const float* __restrict__ boxes, float* __restrict__ dist2_out,
                                                             int32_t* __restrict__ index_out,
                                                             int32_t* __restrict__ scanned_out) {
  __shared__ float4 s_own[kRun];
  __shared__ float4 s_stage[kWaves][kRun];
  __shared__ int s_scanned[kWaves];
  const int run = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t s = int64_t(run) * kRun + threadIdx.x;
  const float4 me = records[s];
  const int my_index = __float_as_int(me.w);
  const bool asks = me.x == me.x;  // false for the NaN records: padding and non-finite points
  s_own[threadIdx.x] = me;
  __syncthreads();

  BestK<CAP> best;
  best.init();
  if (asks) best.scan(k, s_own, me, my_index);

  Box q = empty_box();
  box_add(q, me.x, me.y, me.z);
  q = wave_box(q);
  const bool wave_asks = __any(asks);
  float wave_worst = wave_max(asks ? best.wd : -INFINITY);
  int scanned = 0;

  // candidates in the order own + 1, own - 1, own + 2, ...: number c is run + (c / 2 + 1) or run - (c / 2 + 1).
  // 64 at a time: lane l tests candidate base + l against the wave's bound, the ballot lists the runs to visit.
  const int candidates = wave_asks ? 2 * (runs - 1) : 0;
  for (int base = 0; base < candidates; base += GS_WAVE) {
    const int c = base + lane, dist = (c >> 1) + 1;
    const int other = (c & 1) ? run - dist : run + dist;
    bool near = false;
    if (other >= 0 && other < runs) near = !(box_dist2(q, boxes + 8 * int64_t(other)) > wave_worst);
    uint64_t todo = __ballot(near);
    while (todo) {  // at most 64 rounds
      const int bit = __builtin_ctzll(todo);
      todo &= todo - 1;
      const int cb = base + bit, db = (cb >> 1) + 1;
      const int cand = (cb & 1) ? run - db : run + db;  // in [0, runs): its lane tested it
      const float* cbox = boxes + 8 * int64_t(cand);
      if (box_dist2(q, cbox) > wave_worst) continue;  // the bound has shrunk since the ballot (wave-uniform)
      ++scanned;
      float4* stage = s_stage[wave];
      const float4* src = records + int64_t(cand) * kRun;
#pragma unroll
      for (int part = 0; part < kRun / GS_WAVE; ++part) stage[part * GS_WAVE + lane] = src[part * GS_WAVE + lane];
      // the wave's own LDS writes before its reads: LDS operations of one wave complete in order; the fence keeps the
      // compiler from moving them across
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      Box p = empty_box();
      box_add(p, me.x, me.y, me.z);
      if (asks && !(box_dist2(p, cbox) > best.wd)) best.scan(k, stage, me, my_index);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // every lane is done reading before the next staging overwrites
      wave_worst = wave_max(asks ? best.wd : -INFINITY);
    }
  }

  if (s < n) {  // my_index is a row of the outputs
    float* d_row = dist2_out + int64_t(my_index) * k;
    int32_t* j_row = index_out ? index_out + int64_t(my_index) * k : nullptr;
#pragma unroll
    for (int i = 0; i < CAP; ++i)
      if (i < k) {
        d_row[i] = best.d[i];
        if (j_row) j_row[i] = best.j[i] == kNoIndex ? -1 : best.j[i];
      }
  }
  // diagnostic: (wave, run) pairs scanned by this workgroup
  if (lane == 0) s_scanned[wave] = scanned;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) total += s_scanned[w];
    scanned_out[run] = total;
  }
}

// --------------------------------------------------------------------------------------------------- scratch layout
struct Layout {
  int64_t runs, scanned, partials, codes_in, order_in, codes_out, order_out, records, boxes, sort, sort_bytes, total;
};

Layout knn_layout(int64_t n) {
  Layout l{};
  l.runs = gs_div_up(n, kRun);
  int64_t at = 0;
  auto take = [&at](int64_t bytes) {
    const int64_t here = at;
    at += gs_align_up(bytes, 256);
    return here;
  };
  l.scanned = take(l.runs * 4);  // first, so that a caller can read it: see include/gsplat_hip.h
  l.partials = take(kMaxPartials * 8 * 4);
  l.codes_in = take(n * 8);
  l.order_in = take(n * 4);
  l.codes_out = take(n * 8);
  l.order_out = take(n * 4);
  l.records = take(l.runs * kRun * 16);
  l.boxes = take(l.runs * 8 * 4);
  l.sort_bytes = gs_sort_scratch_bytes(n, 8);
  l.sort = take(l.sort_bytes);
  l.total = at;
  return l;
}

}  // namespace

extern "C" int64_t gs_knn3d_scratch_bytes(int64_t n) {
  if (n <= 0) return 0;
  return knn_layout(n).total;
}

extern "C" int gs_knn3d(int64_t n, const float* points, int32_t k, float* dist2, int32_t* index, void* scratch,
                        int64_t scratch_bytes, void* stream) {
  GS_REQUIRE(n >= 0 && n < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT, "gs_knn3d: %lld points (0 .. 2^31 - 1)",
             (long long)n);
  GS_REQUIRE(k >= 1 && k <= GS_KNN_MAX, GS_ERR_INVALID_ARGUMENT, "gs_knn3d: k %d not in [1,%d]", k, GS_KNN_MAX);
  if (n == 0) return GS_OK;
  GS_REQUIRE(points && dist2 && scratch, GS_ERR_INVALID_ARGUMENT, "gs_knn3d: NULL buffer (%s)",
             !points ? "points" : !dist2 ? "dist2" : "scratch");
  const Layout l = knn_layout(n);
  GS_REQUIRE(scratch_bytes >= l.total, GS_ERR_SCRATCH_TOO_SMALL, "gs_knn3d: scratch of %lld bytes, %lld needed",
             (long long)scratch_bytes, (long long)l.total);
  GS_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, GS_ERR_INVALID_ARGUMENT,
             "gs_knn3d: scratch is not 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* p = static_cast<char*>(scratch);
  int32_t* scanned = reinterpret_cast<int32_t*>(p + l.scanned);
  float* partials = reinterpret_cast<float*>(p + l.partials);
  uint64_t* codes_in = reinterpret_cast<uint64_t*>(p + l.codes_in);
  int32_t* order_in = reinterpret_cast<int32_t*>(p + l.order_in);
  uint64_t* codes_out = reinterpret_cast<uint64_t*>(p + l.codes_out);
  int32_t* order_out = reinterpret_cast<int32_t*>(p + l.order_out);
  float4* records = reinterpret_cast<float4*>(p + l.records);
  float* boxes = reinterpret_cast<float*>(p + l.boxes);
  const unsigned runs = unsigned(l.runs);
  const unsigned num_partials = runs < unsigned(kMaxPartials) ? runs : unsigned(kMaxPartials);

  hipLaunchKernelGGL(knn_bbox_kernel, dim3(num_partials), dim3(kThreads), 0, s, n, points, partials);
  hipLaunchKernelGGL(knn_codes_kernel, dim3(runs), dim3(kThreads), 0, s, n, points, partials, int(num_partials),
                     codes_in, order_in);
  if (int rc = gs_radix_sort_pairs(n, 8, codes_in, order_in, codes_out, order_out, 0, 3 * kCodeBits, p + l.sort,
                                   l.sort_bytes, s))
    return rc;
  hipLaunchKernelGGL(knn_gather_kernel, dim3(runs), dim3(kThreads), 0, s, n, points, order_out, records, boxes);
  if (k <= 4)
    hipLaunchKernelGGL(knn_query_kernel<4>, dim3(runs), dim3(kThreads), 0, s, n, int(runs), int(k), records, boxes,
                       dist2, index, scanned);
  else
    hipLaunchKernelGGL(knn_query_kernel<GS_KNN_MAX>, dim3(runs), dim3(kThreads), 0, s, n, int(runs), int(k), records,
                       boxes, dist2, index, scanned);
  GS_CHECK_LAUNCH("gs_knn3d");
  return GS_OK;
}
