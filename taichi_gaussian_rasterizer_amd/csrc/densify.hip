// densify.hip -- changing the number of Gaussians on the device: which rows go where (plan), every per-row table moved
// by that plan in one launch (move_rows), the children of a 3D split, and the per-row statistics a trainer thresholds.
//   plan        three byte masks -> src_of: the source row of every output row, in a fixed order (kept rows ascending,
//               then the clones ascending, then the children parent-major) + the four counts.  A counting pass per
//               workgroup of 2048 rows, ONE gs_full_cumsum_i32 over the 3 x workgroups counts (kept | clones | split
//               parents, so the three prefixes come from one scan), an emit pass.  No atomics: the plan is a function
//               of the masks.
//   move_rows   dst[j] = src[src_of[j]] (or zero from copy_rows on) for up to 32 columns at once, as bytes.
//   split3d     child position = parent + R(q / |q|) (exp(log_scaling) * noise), child log_scaling = parent - log_shrink
//   accumulate  stats[row] += (seen, |d mean|, prune cost, split score, visibility), max(radius), rows of one view

#include "gs_common.h"

namespace {

constexpr int kThreads = 256;

// ---------------------------------------------------------------------------------------------------------- plan
constexpr int kRowsPerThread = 8;
constexpr int kRowsPerBlock = kThreads * kRowsPerThread;  // 2048

struct PlanArgs {
  int64_t n;
  const uint8_t* prune;
  const uint8_t* split;
  const uint8_t* clone;
  int children;
  int64_t capacity;
  int nb;  // workgroups = ceil(n / 2048)
};

// bit k: mask[i0 + k] != 0 for the rows of [i0, i0 + 8) below n.  i0 is a multiple of 8, so an 8-byte aligned mask is
// read with one 8-byte load.
__device__ __forceinline__ unsigned mask_bits8(const uint8_t* __restrict__ mask, int64_t i0, int64_t n) {
  if (!mask || i0 >= n) return 0u;
  unsigned bits = 0;
  if (i0 + 8 <= n && (reinterpret_cast<uintptr_t>(mask) & 7) == 0) {
    const uint2 w = *reinterpret_cast<const uint2*>(mask + i0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      bits |= unsigned(((w.x >> (8 * k)) & 0xffu) != 0) << k;
      bits |= unsigned(((w.y >> (8 * k)) & 0xffu) != 0) << (4 + k);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (i0 + k < n) bits |= unsigned(mask[i0 + k] != 0) << k;
  }
  return bits;
}

// the three classes of the thread's 8 rows: kept = neither pruned nor split (a cloned row is kept), clones, split parents
struct RowBits {
  unsigned kept, clone, split;
};
__device__ __forceinline__ RowBits classify8(const PlanArgs& a, int64_t i0) {
  const unsigned live = i0 >= a.n ? 0u : (a.n - i0 >= 8 ? 0xffu : (1u << int(a.n - i0)) - 1u);
  const unsigned p = mask_bits8(a.prune, i0, a.n);
  const unsigned s = mask_bits8(a.split, i0, a.n) & ~p;
  const unsigned c = mask_bits8(a.clone, i0, a.n) & ~p & ~s;
  return RowBits{live & ~p & ~s, c, s};
}

// exclusive prefix of `mine` over the workgroup and the workgroup's total (one barrier; s_cnt: one int per wave)
__device__ __forceinline__ int block_prefix(int mine, int* s_cnt, int& total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int incl = mine;
#pragma unroll
  for (int off = 1; off < GS_WAVE; off <<= 1) {
    const int up = __shfl_up(incl, off);
    if (lane >= off) incl += up;
  }
  if (lane == GS_WAVE - 1) s_cnt[wave] = incl;
  __syncthreads();
  int before = incl - mine;
  total = 0;
#pragma unroll
  for (int w = 0; w < kThreads / GS_WAVE; ++w) {
    before += w < wave ? s_cnt[w] : 0;
    total += s_cnt[w];
  }
  return before;
}

// counts (3, nb): kept | clones | split parents of every workgroup's 2048 rows
__global__ __launch_bounds__(kThreads) void plan_count_kernel(PlanArgs a, int* counts) {
  __shared__ int s_cnt[3][kThreads / GS_WAVE];
  const int64_t i0 = (int64_t(blockIdx.x) * kThreads + threadIdx.x) * kRowsPerThread;
  const RowBits r = classify8(a, i0);
  int tk, tc, ts;
  block_prefix(__popc(r.kept), s_cnt[0], tk);
  block_prefix(__popc(r.clone), s_cnt[1], tc);
  block_prefix(__popc(r.split), s_cnt[2], ts);
  if (threadIdx.x == 0) {
    counts[blockIdx.x] = tk;
    counts[a.nb + blockIdx.x] = tc;
    counts[2 * a.nb + blockIdx.x] = ts;
  }
}

// prefix (3 nb + 1): the full cumsum of counts, so prefix[nb] = all kept rows, prefix[2 nb] - prefix[nb] = all clones
__global__ __launch_bounds__(kThreads) void plan_emit_kernel(PlanArgs a, const int* prefix, int32_t* src_of,
                                                             int32_t* out_counts) {
  __shared__ int s_cnt[3][kThreads / GS_WAVE];
  const int64_t i0 = (int64_t(blockIdx.x) * kThreads + threadIdx.x) * kRowsPerThread;
  const RowBits r = classify8(a, i0);
  int tk, tc, ts;
  const int bk = block_prefix(__popc(r.kept), s_cnt[0], tk);
  const int bc = block_prefix(__popc(r.clone), s_cnt[1], tc);
  const int bs = block_prefix(__popc(r.split), s_cnt[2], ts);
  const int64_t kept = prefix[a.nb], clones = prefix[2 * a.nb] - prefix[a.nb];
  const int64_t parents = prefix[3 * a.nb] - prefix[2 * a.nb];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out_counts[0] = int32_t(kept);
    out_counts[1] = int32_t(clones);
    out_counts[2] = int32_t(parents);
    out_counts[3] = int32_t(kept + clones + a.children * parents);
  }
  int64_t at = int64_t(prefix[blockIdx.x]) + bk;
  for (unsigned bits = r.kept; bits; bits &= bits - 1, ++at)
    if (at < a.capacity) src_of[at] = int32_t(i0 + __ffs(bits) - 1);
  at = kept + (prefix[a.nb + blockIdx.x] - prefix[a.nb]) + bc;
  for (unsigned bits = r.clone; bits; bits &= bits - 1, ++at)
    if (at < a.capacity) src_of[at] = int32_t(i0 + __ffs(bits) - 1);
  at = kept + clones + (int64_t(prefix[2 * a.nb + blockIdx.x] - prefix[2 * a.nb]) + bs) * a.children;
  for (unsigned bits = r.split; bits; bits &= bits - 1) {
    const int32_t row = int32_t(i0 + __ffs(bits) - 1);
    for (int c = 0; c < a.children; ++c, ++at)
      if (at < a.capacity) src_of[at] = row;
  }
}

int64_t plan_blocks(int64_t n) { return gs_div_up(n, kRowsPerBlock); }
int64_t plan_counts_bytes(int64_t n) { return gs_align_up((3 * plan_blocks(n) + 1) * 4, 256); }

// ---------------------------------------------------------------------------------------------------------- move
// One launch for all columns: blockIdx.y = the column, the workgroups of a column stride over its units.  A unit is
// 16 bytes of an output row where the column's row size and both of its pointers are multiples of 16, else 4 bytes;
// neighbouring lanes take neighbouring units, so a source row is read as one run of bytes and the output is written
// as one stream.  Columns differ in size by two orders of magnitude (192-byte SH rows, 4-byte opacities): a workgroup
// whose first unit lies behind its column's last one leaves at once.
constexpr int kMoveMaxBlocks = 2048;  // per column: 256 CUs x 8 workgroups, the rest by grid stride

struct MoveArgs {
  int64_t rows;
  const int32_t* src_of;
  GsMoveColumn col[GS_MOVE_COLUMNS_MAX];
};

// unit counts are 32-bit (the host refuses a column of 2^32 units or more), so u / per_row is the 32-bit division
template <typename Unit>
__device__ __forceinline__ void move_units(const GsMoveColumn& c, const int32_t* __restrict__ src_of, int64_t rows) {
  const uint32_t per_row = uint32_t(c.row_bytes) / uint32_t(sizeof(Unit));
  const uint32_t total = uint32_t(rows) * per_row;
  const uint32_t copy_units = uint32_t(c.copy_rows) * per_row;
  const Unit* __restrict__ src = static_cast<const Unit*>(c.src);
  Unit* __restrict__ dst = static_cast<Unit*>(c.dst);
  const uint32_t step = gridDim.x * kThreads;
  // u + step stays below 2^32: the host checks total + step
  for (uint32_t u = blockIdx.x * kThreads + threadIdx.x; u < total; u += step) {
    Unit v{};
    if (u < copy_units) {
      const uint32_t j = u / per_row;
      v = src[int64_t(src_of[j]) * per_row + (u - j * per_row)];
    }
    dst[u] = v;
  }
}

__global__ __launch_bounds__(kThreads) void move_rows_kernel(MoveArgs a) {
  const GsMoveColumn& c = a.col[blockIdx.y];
  const bool wide = ((reinterpret_cast<uintptr_t>(c.src) | reinterpret_cast<uintptr_t>(c.dst) |
                      uintptr_t(c.row_bytes)) & 15) == 0;
  if (wide) move_units<uint4>(c, a.src_of, a.rows);
  else move_units<uint32_t>(c, a.src_of, a.rows);
}

// ---------------------------------------------------------------------------------------------------------- split
struct SplitArgs {
  int64_t count;
  const int32_t* parent_of;
  const float* position;
  const float* log_scaling;
  const float* rotation;
  const float* noise;
  float log_shrink;
  float* child_position;
  float* child_log_scaling;
};

__global__ __launch_bounds__(kThreads) void split3d_kernel(SplitArgs a) {
  const int64_t t = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (t >= a.count) return;
  const int64_t p = a.parent_of[t];
  const float* q = a.rotation + 4 * p;  // xyzw, as project_math.h reads it
  const float qlen = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const float x = q[0] / qlen, y = q[1] / qlen, z = q[2] / qlen, w = q[3] / qlen;
  float ls[3], d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ls[k] = a.log_scaling[3 * p + k];
    d[k] = expf(ls[k]) * a.noise[3 * t + k];
  }
  const float x2 = x * x, y2 = y * y, z2 = z * z;
  const float R[3][3] = {{1 - 2 * y2 - 2 * z2, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y},
                         {2 * x * y + 2 * w * z, 1 - 2 * x2 - 2 * z2, 2 * y * z - 2 * w * x},
                         {2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x2 - 2 * y2}};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float centre = a.position[3 * p + r];
    const float offset = R[r][0] * d[0] + R[r][1] * d[1] + R[r][2] * d[2];
    // zero noise leaves the parent's bits (-0.0f + 0.0f would be +0.0f)
    a.child_position[3 * t + r] = offset == 0.0f ? centre : centre + offset;
    a.child_log_scaling[3 * t + r] = ls[r] - a.log_shrink;
  }
}

// ---------------------------------------------------------------------------------------------------------- stats
struct StatsArgs {
  int64_t n, v;
  const int64_t* points_in_view;
  const float* grad2d;
  int grad2d_stride;
  const float* heuristic;
  const float* visibility;
  const float* gaussians2d;
  float* stats;
};

// sqrt(x^2 + y^2) on operands scaled by a power of two, so that the squares of small gradients (below 2^-63) do not
// underflow: the scaling is exact, the result that of the unscaled formula wherever that neither under- nor overflows
__device__ __forceinline__ float length2(float x, float y) {
  const float m = fmaxf(fabsf(x), fabsf(y));
  if (!(m > 0.0f) || isinf(m)) return sqrtf(x * x + y * y);  // zeros, infinities and NaNs as they come
  const int e = ilogbf(m);
  x = ldexpf(x, -e);
  y = ldexpf(y, -e);
  return ldexpf(sqrtf(x * x + y * y), e);
}

// the rows of a view are distinct: plain read-modify-write, one lane per listed row
__global__ __launch_bounds__(kThreads) void stats_kernel(StatsArgs a) {
  const int64_t t = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (t >= a.v) return;
  const int64_t row = a.points_in_view[t];
  if (row < 0 || row >= a.n) return;
  float* s = a.stats + row * GS_DENSIFY_STATS;
  const float vis = a.visibility ? a.visibility[t] : 0.0f;
  if (!a.visibility || vis > 0.0f) s[0] += 1.0f;
  if (a.grad2d) {
    s[1] += length2(a.grad2d[t * a.grad2d_stride], a.grad2d[t * a.grad2d_stride + 1]);
  }
  if (a.heuristic) {
    s[2] += a.heuristic[2 * t];
    s[3] += a.heuristic[2 * t + 1];
  }
  if (a.visibility) s[4] += vis;
  if (a.gaussians2d) {  // packed splat: mean 0:2, axis 2:4, sigma 4:6, alpha 6
    const float radius = fmaxf(a.gaussians2d[7 * t + 4], a.gaussians2d[7 * t + 5]);
    s[5] = fmaxf(s[5], radius);
  }
}

}  // namespace

extern "C" int64_t gs_densify_plan_scratch_bytes(int64_t n) {
  if (n <= 0) return 0;
  return 2 * plan_counts_bytes(n) + gs_cumsum_scratch_bytes(3 * plan_blocks(n));
}

extern "C" int gs_densify_plan(int64_t n, const uint8_t* prune, const uint8_t* split, const uint8_t* clone,
                               int32_t children, int64_t capacity, int32_t* src_of, int32_t* counts, void* scratch,
                               int64_t scratch_bytes, void* stream) {
  GS_REQUIRE(children >= 1 && children <= GS_DENSIFY_CHILDREN_MAX, GS_ERR_INVALID_ARGUMENT,
             "gs_densify_plan: children %d not in [1,%d]", children, GS_DENSIFY_CHILDREN_MAX);
  GS_REQUIRE(n >= 0 && n * (children > 2 ? children : 2) < (int64_t(1) << 31) && n < (int64_t(1) << 31),
             GS_ERR_INVALID_ARGUMENT, "gs_densify_plan: %lld rows with %d children (n * max(2, children) must stay "
             "below 2^31)", (long long)n, children);
  GS_REQUIRE(capacity >= 0, GS_ERR_INVALID_ARGUMENT, "gs_densify_plan: capacity %lld", (long long)capacity);
  if (n == 0) return GS_OK;
  GS_REQUIRE(counts && (src_of || capacity == 0), GS_ERR_INVALID_ARGUMENT, "gs_densify_plan: NULL buffer");
  GS_REQUIRE(scratch && scratch_bytes >= gs_densify_plan_scratch_bytes(n), GS_ERR_SCRATCH_TOO_SMALL,
             "gs_densify_plan: scratch of %lld bytes, %lld needed", (long long)scratch_bytes,
             (long long)gs_densify_plan_scratch_bytes(n));
  GS_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, GS_ERR_INVALID_ARGUMENT,
             "gs_densify_plan: scratch is not 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nb = int(plan_blocks(n));
  const PlanArgs a{n, prune, split, clone, children, capacity, nb};
  char* p = static_cast<char*>(scratch);
  int* block_counts = reinterpret_cast<int*>(p);
  int* prefix = reinterpret_cast<int*>(p + plan_counts_bytes(n));
  void* scan_scratch = p + 2 * plan_counts_bytes(n);
  hipLaunchKernelGGL(plan_count_kernel, dim3(unsigned(nb)), dim3(kThreads), 0, s, a, block_counts);
  if (int rc = gs_full_cumsum_i32(3 * int64_t(nb), block_counts, prefix, scan_scratch,
                                  gs_cumsum_scratch_bytes(3 * int64_t(nb)), s))
    return rc;
  hipLaunchKernelGGL(plan_emit_kernel, dim3(unsigned(nb)), dim3(kThreads), 0, s, a, prefix, src_of, counts);
  GS_CHECK_LAUNCH("gs_densify_plan");
  return GS_OK;
}

extern "C" int gs_table_move_rows(int64_t rows, const int32_t* src_of, int32_t columns,
                                  const GsMoveColumn* columns_host, void* stream) {
  GS_REQUIRE(rows >= 0 && rows < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT, "gs_table_move_rows: %lld rows",
             (long long)rows);
  GS_REQUIRE(columns >= 0 && columns <= GS_MOVE_COLUMNS_MAX, GS_ERR_INVALID_ARGUMENT,
             "gs_table_move_rows: columns %d not in [0,%d]", columns, GS_MOVE_COLUMNS_MAX);
  if (rows == 0 || columns == 0) return GS_OK;
  GS_REQUIRE(columns_host, GS_ERR_INVALID_ARGUMENT, "gs_table_move_rows: NULL buffer (columns)");
  MoveArgs a{};
  a.rows = rows;
  a.src_of = src_of;
  int64_t most_units = 0;
  bool reads = false;
  for (int k = 0; k < columns; ++k) {
    const GsMoveColumn& c = columns_host[k];
    GS_REQUIRE(c.row_bytes >= 4 && c.row_bytes % 4 == 0, GS_ERR_INVALID_ARGUMENT,
               "gs_table_move_rows: column %d has rows of %d bytes (a positive multiple of 4)", k, c.row_bytes);
    GS_REQUIRE(c.copy_rows >= 0 && c.copy_rows <= rows, GS_ERR_INVALID_ARGUMENT,
               "gs_table_move_rows: column %d copies %lld of %lld rows", k, (long long)c.copy_rows, (long long)rows);
    GS_REQUIRE(c.dst && (c.src || c.copy_rows == 0), GS_ERR_INVALID_ARGUMENT,
               "gs_table_move_rows: NULL buffer (column %d)", k);
    GS_REQUIRE(((reinterpret_cast<uintptr_t>(c.src) | reinterpret_cast<uintptr_t>(c.dst)) & 3) == 0,
               GS_ERR_INVALID_ARGUMENT, "gs_table_move_rows: column %d is not 4-byte aligned", k);
    a.col[k] = c;
    const bool wide = ((reinterpret_cast<uintptr_t>(c.src) | reinterpret_cast<uintptr_t>(c.dst) |
                        uintptr_t(c.row_bytes)) & 15) == 0;
    const int64_t units = rows * (c.row_bytes / (wide ? 16 : 4));
    most_units = units > most_units ? units : most_units;
    reads = reads || c.copy_rows > 0;
  }
  GS_REQUIRE(src_of || !reads, GS_ERR_INVALID_ARGUMENT, "gs_table_move_rows: NULL buffer (src_of)");
  const int64_t blocks = gs_div_up(most_units, kThreads);
  const unsigned grid_x = unsigned(blocks < kMoveMaxBlocks ? blocks : kMoveMaxBlocks);
  const dim3 grid(grid_x, unsigned(columns));
  hipStream_t s = static_cast<hipStream_t>(stream);
  GS_REQUIRE(most_units + int64_t(grid_x) * kThreads < (int64_t(1) << 32), GS_ERR_UNSUPPORTED,
             "gs_table_move_rows: a column of %lld units of 4 or 16 bytes (below 2^32 less one grid stride)",
             (long long)most_units);
  hipLaunchKernelGGL(move_rows_kernel, grid, dim3(kThreads), 0, s, a);
  GS_CHECK_LAUNCH("gs_table_move_rows");
  return GS_OK;
}

extern "C" int gs_split3d_children(int64_t count, int32_t children, const int32_t* parent_of, const float* position,
                                   const float* log_scaling, const float* rotation, const float* noise,
                                   double log_shrink, float* child_position, float* child_log_scaling, void* stream) {
  GS_REQUIRE(children >= 1 && children <= GS_DENSIFY_CHILDREN_MAX, GS_ERR_INVALID_ARGUMENT,
             "gs_split3d_children: children %d not in [1,%d]", children, GS_DENSIFY_CHILDREN_MAX);
  GS_REQUIRE(count >= 0 && count < (int64_t(1) << 31) && count % children == 0, GS_ERR_INVALID_ARGUMENT,
             "gs_split3d_children: %lld rows for %d children per parent", (long long)count, children);
  if (count == 0) return GS_OK;
  GS_REQUIRE(parent_of && position && log_scaling && rotation && noise && child_position && child_log_scaling,
             GS_ERR_INVALID_ARGUMENT, "gs_split3d_children: NULL buffer");
  const SplitArgs a{count, parent_of, position, log_scaling, rotation, noise, float(log_shrink), child_position,
                    child_log_scaling};
  hipLaunchKernelGGL(split3d_kernel, dim3(unsigned(gs_div_up(count, kThreads))), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), a);
  GS_CHECK_LAUNCH("gs_split3d_children");
  return GS_OK;
}

extern "C" int gs_densify_accumulate(int64_t n, int64_t v, const int64_t* points_in_view, const float* grad2d,
                                     int32_t grad2d_stride, const float* heuristic, const float* visibility,
                                     const float* gaussians2d, float* stats, void* stream) {
  GS_REQUIRE(n >= 0 && n < (int64_t(1) << 31) && v >= 0 && v < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT,
             "gs_densify_accumulate: %lld listed rows of %lld", (long long)v, (long long)n);
  GS_REQUIRE(!grad2d || grad2d_stride >= 2, GS_ERR_INVALID_ARGUMENT,
             "gs_densify_accumulate: grad2d has a stride of %d floats (at least 2)", grad2d_stride);
  if (n == 0 || v == 0) return GS_OK;
  GS_REQUIRE(points_in_view && stats, GS_ERR_INVALID_ARGUMENT, "gs_densify_accumulate: NULL buffer");
  const StatsArgs a{n, v, points_in_view, grad2d, grad2d_stride, heuristic, visibility, gaussians2d, stats};
  hipLaunchKernelGGL(stats_kernel, dim3(unsigned(gs_div_up(v, kThreads))), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), a);
  GS_CHECK_LAUNCH("gs_densify_accumulate");
  return GS_OK;
}
