// rows.hip -- row lists of several views: what an optimizer step over a BATCH of views needs in place of a sort.
// Each view's backward lists its visible rows ascending and distinct (points_in_view), so the index list of a gradient
// summed over B backward passes is a concatenation of at most B strictly ascending runs, however autograd laid the sum
// out.  Three operations over such lists:
//   find_runs   where the runs start (a run starts at 0 and at every i with rows[i] <= rows[i-1])
//   sum_runs    for each row of a step, the sum in run order of the value rows that list it: one binary search per
//               run, then the hit rows added in run order -- a fixed order, so the same bits on every call
//   union       the ascending distinct union of the views' lists through a bitmap over the N rows
// Index lists are 8 MB per view at V = 1 M and stay cache-resident under the searches; the value rows are read once.
// A batch rendered as one node (render_views) has every view's slot_of table (n int32: the compact row of Gaussian i in
// that view, or -1) and needs neither runs nor searches:
//   views_union     the same bitmap built from the tables in one streaming pass, without atomics
//   views_sum_rows  sum_runs with the binary search replaced by one table read per view

#include "gs_common.h"

namespace {

constexpr int kThreads = 256;

// ---------------------------------------------------------------------------------------------------- find_runs
__global__ void runs_init_kernel(int64_t count, int max_runs, int64_t* run_starts, int* run_count) {
  const int t = threadIdx.x;
  if (t <= max_runs) run_starts[t] = t == 0 ? 0 : count;
  if (t == 0) *run_count = 1;  // the run that starts at 0
}

// Every start behind the first is an element not above its predecessor.  The count is one atomic add per workgroup that
// holds a start.  The starts have to come out ASCENDING, which an atomic append does not give: slots[0 .. K) is kept as
// the K smallest starts seen, ascending, by an insertion that pushes a value down the slots with one atomicMin per slot
// -- a slot keeps the smaller value, the larger one moves on.  Every value enters at slot 0, which therefore ends as
// the smallest of all; everything but that one reaches slot 1, and so on: the end state does not depend on the order
// in which the workgroups arrive.  Slots start at `count`, which is above every start.  Only the first K starts of a
// workgroup can be among the K smallest, and a start not below the last slot cannot be either (slots only fall).
__global__ __launch_bounds__(kThreads) void runs_find_kernel(int64_t count, const int64_t* rows, int K,
                                                             unsigned long long* slots, int* run_count) {
  __shared__ int s_cnt[kThreads / GS_WAVE];
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  const bool start = i >= 1 && i < count && rows[i] <= rows[i - 1];
  const uint64_t b = __ballot(start);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) s_cnt[wave] = __popcll(b);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kThreads / GS_WAVE; ++w) {
    before += w < wave ? s_cnt[w] : 0;
    total += s_cnt[w];
  }
  if (threadIdx.x == 0 && total > 0) atomicAdd(run_count, total);
  if (!start || before + __popcll(b & ((1ull << lane) - 1ull)) >= K) return;
  unsigned long long x = (unsigned long long)i;
  if (x >= __atomic_load_n(&slots[K - 1], __ATOMIC_RELAXED)) return;
  const unsigned long long none = (unsigned long long)count;
  for (int k = 0; k < K; ++k) {
    const unsigned long long old = atomicMin(&slots[k], x);
    if (old == none) break;      // the slot was free: nothing to move on
    x = old > x ? old : x;
  }
}

// ---------------------------------------------------------------------------------------------------- sum_runs
struct SumArgs {
  int64_t rows;
  const int64_t* indexes;
  int runs;
  const int64_t* run_starts;
  int64_t grad_count;
  const int64_t* grad_indexes;
  int dims;
  const float* grad_values;
  float* out;
};

// position of `want` in the strictly ascending grad_indexes[lo, end), or -1
__device__ __forceinline__ int find_in_run(const int64_t* __restrict__ g, int64_t lo, int64_t end, int64_t want) {
  int64_t hi = end;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (g[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  return (lo < end && g[lo] == want) ? int(lo) : -1;
}

__device__ __forceinline__ int64_t clamp_start(int64_t s, int64_t count) { return s < 0 ? 0 : (s > count ? count : s); }

template <int VEC> struct Piece;
template <> struct Piece<1> { typedef float T; };
template <> struct Piece<4> { typedef float4 T; };
__device__ __forceinline__ float piece_zero(float) { return 0.0f; }
__device__ __forceinline__ float4 piece_zero(float4) { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float piece_add(float a, float b) { return a + b; }
__device__ __forceinline__ float4 piece_add(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// The second half of a wide-row sum.  A wave holds 64 / RL consecutive output rows from row0 on; lane j * RL + r holds
// in `hit` the value row that source r (a run, a view) has for the wave's row j, or -1.  The hits are handed around by
// cross-lane reads: the lanes stride over the (row, piece) pairs of the wave's rows -- a piece is VEC floats, `pieces`
// of them per row -- load every source's piece and then add the hit ones in source order from zero.  row_of(r, at):
// the first piece of value row `at` of source r.  Neighbouring lanes read neighbouring pieces of one value row, so a
// value row is read as one contiguous run of bytes, and the wave's output is one contiguous block.
template <int RL, int VEC, class RowOf>
__device__ __forceinline__ void wave_sum_pieces(int hit, int lane, int64_t row0, int64_t rows, int pieces,
                                                float* out_rows, RowOf row_of) {
  typedef typename Piece<VEC>::T P;
  constexpr int RPW = GS_WAVE / RL;                 // rows per wave
  const int64_t left = rows - row0;
  const int here = int(left < RPW ? left : RPW);    // rows of this wave
  const int units = here * pieces;
  P* out = reinterpret_cast<P*>(out_rows) + row0 * pieces;
  for (int e0 = 0; e0 < units; e0 += GS_WAVE) {     // wave-uniform trip count: the cross-lane reads see every lane
    const int e = e0 + lane;
    const bool live = e < units;
    const int slot = live ? e / pieces : 0;
    const int c = e - slot * pieces;
    P v[RL];
    int at[RL];
#pragma unroll
    for (int r = 0; r < RL; ++r) {
      at[r] = __shfl(hit, slot * RL + r);
      if (!live) at[r] = -1;
      v[r] = piece_zero(P());
      if (at[r] >= 0) v[r] = row_of(r, at[r])[c];
    }
    P acc = piece_zero(P());
#pragma unroll
    for (int r = 0; r < RL; ++r)
      if (at[r] >= 0) acc = piece_add(acc, v[r]);
    if (live) out[e] = acc;
  }
}

// Wide rows.  A wave takes 64 / RL consecutive rows of `indexes`; RL lanes per row (RL >= runs) search one run each, so
// all searches of the wave's rows proceed side by side; wave_sum_pieces then adds the hit rows in run order.
template <int RL, int VEC>
__global__ __launch_bounds__(kThreads) void rows_sum_wide_kernel(SumArgs a) {
  typedef typename Piece<VEC>::T P;
  constexpr int RPW = GS_WAVE / RL;  // rows per wave
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t(blockIdx.x) * kThreads + threadIdx.x) >> 6;
  const int64_t row0 = wave * RPW;
  if (row0 >= a.rows) return;  // the whole wave
  int hit = -1;
  {
    const int64_t i = row0 + lane / RL;
    const int r = lane % RL;
    if (i < a.rows && r < a.runs) {
      const int64_t lo = clamp_start(a.run_starts[r], a.grad_count);
      const int64_t end = clamp_start(a.run_starts[r + 1], a.grad_count);
      hit = find_in_run(a.grad_indexes, lo, end, a.indexes[i]);
    }
  }
  const P* __restrict__ values = reinterpret_cast<const P*>(a.grad_values);
  const int pieces = a.dims / VEC;
  wave_sum_pieces<RL, VEC>(hit, lane, row0, a.rows, pieces, a.out,
                           [&](int, int at) { return values + int64_t(at) * pieces; });
}

// Narrow rows (1 to 4 floats): a lane per row, its runs searched one after the other; V4: 16-byte accesses for D = 4.
template <int D, bool V4>
__global__ __launch_bounds__(kThreads) void rows_sum_narrow_kernel(SumArgs a) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= a.rows) return;
  const int64_t want = a.indexes[i];
  float acc[D];
#pragma unroll
  for (int j = 0; j < D; ++j) acc[j] = 0.0f;
  int64_t lo = a.runs > 0 ? clamp_start(a.run_starts[0], a.grad_count) : 0;
  for (int r = 0; r < a.runs; ++r) {
    const int64_t end = clamp_start(a.run_starts[r + 1], a.grad_count);
    const int at = find_in_run(a.grad_indexes, lo, end, want);
    if (at >= 0) {
      if (V4) {
        const float4 v = reinterpret_cast<const float4*>(a.grad_values)[at];
        acc[0] += v.x; acc[1 % D] += v.y; acc[2 % D] += v.z; acc[3 % D] += v.w;
      } else {
#pragma unroll
        for (int j = 0; j < D; ++j) acc[j] += a.grad_values[int64_t(at) * D + j];
      }
    }
    lo = end;
  }
  if (V4) {
    reinterpret_cast<float4*>(a.out)[i] = make_float4(acc[0], acc[1 % D], acc[2 % D], acc[3 % D]);
  } else {
#pragma unroll
    for (int j = 0; j < D; ++j) a.out[i * D + j] = acc[j];
  }
}

template <int RL, int VEC>
void launch_wide(const SumArgs& a, hipStream_t s) {
  const int64_t waves = gs_div_up(a.rows, GS_WAVE / RL);
  hipLaunchKernelGGL((rows_sum_wide_kernel<RL, VEC>), dim3(unsigned(gs_div_up(waves, kThreads / GS_WAVE))),
                     dim3(kThreads), 0, s, a);
}

template <int VEC>
void launch_wide_runs(const SumArgs& a, hipStream_t s) {
  if (a.runs <= 1) launch_wide<1, VEC>(a, s);
  else if (a.runs <= 2) launch_wide<2, VEC>(a, s);
  else if (a.runs <= 4) launch_wide<4, VEC>(a, s);
  else if (a.runs <= 8) launch_wide<8, VEC>(a, s);
  else launch_wide<16, VEC>(a, s);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---------------------------------------------------------------------------------------------------- views_sum_rows
// The same sum with the searches replaced by table reads: view b has its value row of Gaussian i at slot_of_b[i].  For
// ascending `indexes` the slot reads of a view are near-sequential.  The tables travel in the kernel arguments.
struct ViewsArgs {
  int64_t rows;
  const int64_t* indexes;
  int views;
  int dims;
  float* out;
  const int32_t* slot_of[GS_VIEWS_MAX];
  const float* values[GS_VIEWS_MAX];
  int32_t count[GS_VIEWS_MAX];
  int32_t stride[GS_VIEWS_MAX];  // floats; of VEC-float pieces in the VEC = 4 kernels
};

// Wide rows: RL lanes per row (RL >= views) read one view's slot each; a slot outside [0, count) is no hit.
template <int RL, int VEC>
__global__ __launch_bounds__(kThreads) void views_sum_wide_kernel(ViewsArgs a) {
  typedef typename Piece<VEC>::T P;
  constexpr int RPW = GS_WAVE / RL;
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t(blockIdx.x) * kThreads + threadIdx.x) >> 6;
  const int64_t row0 = wave * RPW;
  if (row0 >= a.rows) return;  // the whole wave
  int hit = -1;
  {
    const int64_t i = row0 + lane / RL;
    const int r = lane % RL;
    if (i < a.rows && r < a.views) {
      const int32_t* table = a.slot_of[0];
      int count = a.count[0];
#pragma unroll
      for (int k = 1; k < RL; ++k)  // a select per view: the tables stay in scalar registers
        if (r == k) { table = a.slot_of[k]; count = a.count[k]; }
      const int64_t want = a.indexes[i];
      const int slot = want >= 0 ? table[want] : -1;
      hit = (slot >= 0 && slot < count) ? slot : -1;
    }
  }
  wave_sum_pieces<RL, VEC>(hit, lane, row0, a.rows, a.dims / VEC, a.out, [&](int r, int at) {
    return reinterpret_cast<const P*>(a.values[r]) + int64_t(at) * a.stride[r];
  });
}

// Narrow rows (1 to 4 floats): a lane per row, the views one after the other; V4: 16-byte accesses for D = 4.
template <int D, bool V4>
__global__ __launch_bounds__(kThreads) void views_sum_narrow_kernel(ViewsArgs a) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= a.rows) return;
  const int64_t want = a.indexes[i];
  float acc[D];
#pragma unroll
  for (int j = 0; j < D; ++j) acc[j] = 0.0f;
#pragma unroll
  for (int b = 0; b < GS_VIEWS_MAX; ++b) {
    if (b >= a.views) break;
    const int slot = want >= 0 ? a.slot_of[b][want] : -1;
    if (slot < 0 || slot >= a.count[b]) continue;
    if (V4) {
      const float4 v = reinterpret_cast<const float4*>(a.values[b])[int64_t(slot) * a.stride[b]];
      acc[0] += v.x; acc[1 % D] += v.y; acc[2 % D] += v.z; acc[3 % D] += v.w;
    } else {
#pragma unroll
      for (int j = 0; j < D; ++j) acc[j] += a.values[b][int64_t(slot) * a.stride[b] + j];
    }
  }
  if (V4) {
    reinterpret_cast<float4*>(a.out)[i] = make_float4(acc[0], acc[1 % D], acc[2 % D], acc[3 % D]);
  } else {
#pragma unroll
    for (int j = 0; j < D; ++j) a.out[i * D + j] = acc[j];
  }
}

template <int RL, int VEC>
void launch_views_wide(const ViewsArgs& a, hipStream_t s) {
  const int64_t waves = gs_div_up(a.rows, GS_WAVE / RL);
  hipLaunchKernelGGL((views_sum_wide_kernel<RL, VEC>), dim3(unsigned(gs_div_up(waves, kThreads / GS_WAVE))),
                     dim3(kThreads), 0, s, a);
}

template <int VEC>
void launch_views_wide_lanes(const ViewsArgs& a, hipStream_t s) {
  if (a.views <= 1) launch_views_wide<1, VEC>(a, s);
  else if (a.views <= 2) launch_views_wide<2, VEC>(a, s);
  else if (a.views <= 4) launch_views_wide<4, VEC>(a, s);
  else if (a.views <= 8) launch_views_wide<8, VEC>(a, s);
  else launch_views_wide<16, VEC>(a, s);
}

// ---------------------------------------------------------------------------------------------------- union
// The bitmap: one bit per row of [0, n), in 32-bit words; a thread of the count and emit passes owns 4 words (one
// 16-byte read, 128 rows), a workgroup 1024 words (32768 rows).  scratch = the words, padded to whole workgroups, then
// one int per workgroup: its number of set bits.
constexpr int kWordsPerThread = 4;
constexpr int kWordsPerBlock = kThreads * kWordsPerThread;

int64_t union_blocks(int64_t n) { return gs_div_up(gs_div_up(n, 32), kWordsPerBlock); }
int64_t union_word_bytes(int64_t n) { return union_blocks(n) * kWordsPerBlock * 4; }

__global__ __launch_bounds__(kThreads) void union_mark_kernel(int64_t n, int64_t count, const int64_t* rows,
                                                              unsigned* words) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= count) return;
  const int64_t r = rows[i];
  if (r < 0 || r >= n) return;
  atomicOr(&words[r >> 5], 1u << (r & 31));
}

// The bitmap of the union of several views, from their slot_of tables (n int32 each, negative = not in the view) and
// without atomics: a lane reads VEC consecutive entries of every table (VEC = 4: one 16-byte read), the 32 / VEC
// neighbouring lanes of a word put their bits together by cross-lane ORs and the first of them stores the word.  One
// streaming pass over the tables; every word of the padded bitmap is written, zeros behind row n: nothing to clear.
struct ViewTables {
  int views;
  const int32_t* slot_of[GS_VIEWS_MAX];
};

template <int VEC>
__global__ __launch_bounds__(kThreads) void views_words_kernel(int64_t n, ViewTables t, unsigned* words) {
  constexpr int LPW = 32 / VEC;  // lanes per word
  const int64_t g = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  const int64_t row = g * VEC;
  unsigned bits = 0;
#pragma unroll
  for (int b = 0; b < GS_VIEWS_MAX; ++b) {
    if (b >= t.views) break;
    if (VEC == 4 && row + 3 < n) {
      const int4 s = *reinterpret_cast<const int4*>(t.slot_of[b] + row);
      bits |= unsigned(s.x >= 0) | unsigned(s.y >= 0) << 1 | unsigned(s.z >= 0) << 2 | unsigned(s.w >= 0) << 3;
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if (row + j < n) bits |= unsigned(t.slot_of[b][row + j] >= 0) << j;
    }
  }
  const int lane = threadIdx.x & 63;
  unsigned word = bits << (VEC * (lane % LPW));
#pragma unroll
  for (int off = 1; off < LPW; off <<= 1) word |= __shfl_xor(word, off);  // no lane has left: the grid is whole words
  if (lane % LPW == 0) words[g / LPW] = word;
}

__device__ __forceinline__ int popcount4(const uint4& w) {
  return __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w);
}

// set bits of the workgroup in front of this thread's words and in the whole workgroup (one barrier)
__device__ __forceinline__ void block_scan(int mine, int& before, int& total) {
  __shared__ int s_cnt[kThreads / GS_WAVE];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int incl = mine;
#pragma unroll
  for (int off = 1; off < GS_WAVE; off <<= 1) {
    const int up = __shfl_up(incl, off);
    if (lane >= off) incl += up;
  }
  if (lane == GS_WAVE - 1) s_cnt[wave] = incl;
  __syncthreads();
  before = incl - mine;
  total = 0;
#pragma unroll
  for (int w = 0; w < kThreads / GS_WAVE; ++w) {
    before += w < wave ? s_cnt[w] : 0;
    total += s_cnt[w];
  }
}

__global__ __launch_bounds__(kThreads) void union_count_kernel(const uint4* words, int* block_counts) {
  const uint4 w = words[int64_t(blockIdx.x) * kThreads + threadIdx.x];
  int before, total;
  block_scan(popcount4(w), before, total);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void union_emit_kernel(const uint4* words, const int* block_counts,
                                                              int64_t* union_rows, int* union_count) {
  __shared__ int s_first[kThreads / GS_WAVE];
  const int64_t t = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  const uint4 w = words[t];
  // the set bits of the workgroups in front: every workgroup sums their counts itself
  int first = 0;
  for (int j = threadIdx.x; j < int(blockIdx.x); j += kThreads) first += block_counts[j];
  for (int off = 32; off > 0; off >>= 1) first += __shfl_xor(first, off);
  if ((threadIdx.x & 63) == 0) s_first[threadIdx.x >> 6] = first;
  int before, total;
  block_scan(popcount4(w), before, total);  // its barrier also publishes s_first
  first = 0;
#pragma unroll
  for (int k = 0; k < kThreads / GS_WAVE; ++k) first += s_first[k];
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *union_count = first + total;
  int64_t* out = union_rows + first + before;
  const unsigned part[4] = {w.x, w.y, w.z, w.w};
  const int64_t base = t * (32 * kWordsPerThread);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    unsigned bits = part[k];
    while (bits) {
      const int bit = __ffs(bits) - 1;
      *out++ = base + 32 * k + bit;
      bits &= bits - 1;
    }
  }
}

// the bitmap in `words` (the front of the scratch of n rows) to the ascending list: word-popcount scan, emit
void union_scan_emit(int64_t n, unsigned* words, int64_t* union_rows, int32_t* union_count, hipStream_t s) {
  const int64_t blocks = union_blocks(n);
  int* block_counts = reinterpret_cast<int*>(reinterpret_cast<char*>(words) + union_word_bytes(n));
  hipLaunchKernelGGL(union_count_kernel, dim3(unsigned(blocks)), dim3(kThreads), 0, s,
                     reinterpret_cast<const uint4*>(words), block_counts);
  hipLaunchKernelGGL(union_emit_kernel, dim3(unsigned(blocks)), dim3(kThreads), 0, s,
                     reinterpret_cast<const uint4*>(words), block_counts, union_rows, union_count);
}

}  // namespace

extern "C" int gs_rows_find_runs(int64_t count, const int64_t* rows, int32_t max_runs, int64_t* run_starts,
                                 int32_t* run_count, void* stream) {
  GS_REQUIRE(count >= 0 && count < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT, "gs_rows_find_runs: count %lld",
             (long long)count);
  GS_REQUIRE(max_runs >= 1 && max_runs <= GS_ROWS_MAX_RUNS, GS_ERR_INVALID_ARGUMENT,
             "gs_rows_find_runs: max_runs %d not in [1,%d]", max_runs, GS_ROWS_MAX_RUNS);
  if (count == 0) return GS_OK;
  GS_REQUIRE(rows && run_starts && run_count, GS_ERR_INVALID_ARGUMENT, "gs_rows_find_runs: NULL buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(runs_init_kernel, dim3(1), dim3(GS_WAVE), 0, s, count, max_runs, run_starts, run_count);
  hipLaunchKernelGGL(runs_find_kernel, dim3(unsigned(gs_div_up(count, kThreads))), dim3(kThreads), 0, s, count, rows,
                     max_runs, reinterpret_cast<unsigned long long*>(run_starts + 1), run_count);
  GS_CHECK_LAUNCH("gs_rows_find_runs");
  return GS_OK;
}

extern "C" int gs_rows_sum_runs(int64_t rows, const int64_t* indexes, int32_t runs, const int64_t* run_starts,
                                int64_t grad_count, const int64_t* grad_indexes, int32_t dims,
                                const float* grad_values, float* out, void* stream) {
  GS_REQUIRE(dims >= 1, GS_ERR_INVALID_ARGUMENT, "gs_rows_sum_runs: dims %d", dims);
  GS_REQUIRE(dims <= (1 << 20), GS_ERR_UNSUPPORTED, "gs_rows_sum_runs: rows of %d floats (at most %d)", dims, 1 << 20);
  GS_REQUIRE(rows >= 0 && rows < (int64_t(1) << 31) && grad_count >= 0 && grad_count < (int64_t(1) << 31),
             GS_ERR_INVALID_ARGUMENT, "gs_rows_sum_runs: %lld rows, %lld gradient rows", (long long)rows,
             (long long)grad_count);
  GS_REQUIRE(runs >= 0 && runs <= GS_ROWS_MAX_RUNS, GS_ERR_INVALID_ARGUMENT, "gs_rows_sum_runs: runs %d not in [0,%d]",
             runs, GS_ROWS_MAX_RUNS);
  if (rows == 0) return GS_OK;
  if (grad_count == 0) runs = 0;  // nothing to search: zeros
  GS_REQUIRE(indexes && out && (runs == 0 || (run_starts && grad_indexes && grad_values)), GS_ERR_INVALID_ARGUMENT,
             "gs_rows_sum_runs: NULL buffer");
  const SumArgs a{rows, indexes, runs, run_starts, grad_count, grad_indexes, dims, grad_values, out};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool v4 = dims % 4 == 0 && aligned16(grad_values) && aligned16(out);
  const dim3 lanes(unsigned(gs_div_up(rows, kThreads)));
  if (dims == 1) hipLaunchKernelGGL((rows_sum_narrow_kernel<1, false>), lanes, dim3(kThreads), 0, s, a);
  else if (dims == 2) hipLaunchKernelGGL((rows_sum_narrow_kernel<2, false>), lanes, dim3(kThreads), 0, s, a);
  else if (dims == 3) hipLaunchKernelGGL((rows_sum_narrow_kernel<3, false>), lanes, dim3(kThreads), 0, s, a);
  else if (dims == 4 && v4) hipLaunchKernelGGL((rows_sum_narrow_kernel<4, true>), lanes, dim3(kThreads), 0, s, a);
  else if (dims == 4) hipLaunchKernelGGL((rows_sum_narrow_kernel<4, false>), lanes, dim3(kThreads), 0, s, a);
  else if (v4) launch_wide_runs<4>(a, s);
  else launch_wide_runs<1>(a, s);
  GS_CHECK_LAUNCH("gs_rows_sum_runs");
  return GS_OK;
}

extern "C" int64_t gs_rows_union_scratch_bytes(int64_t n) {
  if (n <= 0) return 0;
  return union_word_bytes(n) + gs_align_up(union_blocks(n) * 4, 256);
}

extern "C" int gs_rows_union(int64_t n, int64_t count, const int64_t* rows, int64_t* union_rows, int32_t* union_count,
                             void* scratch, int64_t scratch_bytes, void* stream) {
  GS_REQUIRE(n >= 0 && n < (int64_t(1) << 31) && count >= 0 && count < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT,
             "gs_rows_union: %lld entries over %lld rows", (long long)count, (long long)n);
  if (n == 0 || count == 0) return GS_OK;
  GS_REQUIRE(rows && union_rows && union_count, GS_ERR_INVALID_ARGUMENT, "gs_rows_union: NULL buffer");
  GS_REQUIRE(scratch && scratch_bytes >= gs_rows_union_scratch_bytes(n), GS_ERR_SCRATCH_TOO_SMALL,
             "gs_rows_union: scratch of %lld bytes, %lld needed", (long long)scratch_bytes,
             (long long)gs_rows_union_scratch_bytes(n));
  GS_REQUIRE(aligned16(scratch), GS_ERR_INVALID_ARGUMENT, "gs_rows_union: scratch is not 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned* words = static_cast<unsigned*>(scratch);
  if (int rc = gs_memset_async(words, size_t(union_word_bytes(n)), s, "gs_rows_union: clearing the bitmap failed")) return rc;
  hipLaunchKernelGGL(union_mark_kernel, dim3(unsigned(gs_div_up(count, kThreads))), dim3(kThreads), 0, s, n, count,
                     rows, words);
  union_scan_emit(n, words, union_rows, union_count, s);
  GS_CHECK_LAUNCH("gs_rows_union");
  return GS_OK;
}

extern "C" int64_t gs_views_union_scratch_bytes(int64_t n) { return gs_rows_union_scratch_bytes(n); }

extern "C" int gs_views_union(int64_t n, int32_t views, const int32_t* const* slot_of_host, int64_t* union_rows,
                              int32_t* union_count, void* scratch, int64_t scratch_bytes, void* stream) {
  GS_REQUIRE(n >= 0 && n < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT, "gs_views_union: %lld rows", (long long)n);
  GS_REQUIRE(views >= 0 && views <= GS_VIEWS_MAX, GS_ERR_INVALID_ARGUMENT, "gs_views_union: views %d not in [0,%d]",
             views, GS_VIEWS_MAX);
  if (n == 0 || views == 0) return GS_OK;
  GS_REQUIRE(slot_of_host && union_rows && union_count, GS_ERR_INVALID_ARGUMENT, "gs_views_union: NULL buffer");
  ViewTables t{};
  t.views = views;
  bool v4 = true;
  for (int b = 0; b < views; ++b) {
    GS_REQUIRE(slot_of_host[b], GS_ERR_INVALID_ARGUMENT, "gs_views_union: NULL buffer (slot_of of view %d)", b);
    t.slot_of[b] = slot_of_host[b];
    v4 = v4 && aligned16(slot_of_host[b]);
  }
  GS_REQUIRE(scratch && scratch_bytes >= gs_views_union_scratch_bytes(n), GS_ERR_SCRATCH_TOO_SMALL,
             "gs_views_union: scratch of %lld bytes, %lld needed", (long long)scratch_bytes,
             (long long)gs_views_union_scratch_bytes(n));
  GS_REQUIRE(aligned16(scratch), GS_ERR_INVALID_ARGUMENT, "gs_views_union: scratch is not 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned* words = static_cast<unsigned*>(scratch);
  const int64_t word_blocks = union_blocks(n) * kWordsPerThread;  // workgroups of one lane per word
  if (v4) hipLaunchKernelGGL(views_words_kernel<4>, dim3(unsigned(word_blocks * 8)), dim3(kThreads), 0, s, n, t, words);
  else hipLaunchKernelGGL(views_words_kernel<1>, dim3(unsigned(word_blocks * 32)), dim3(kThreads), 0, s, n, t, words);
  union_scan_emit(n, words, union_rows, union_count, s);
  GS_CHECK_LAUNCH("gs_views_union");
  return GS_OK;
}

extern "C" int gs_views_sum_rows(int64_t rows, const int64_t* indexes, int32_t views, const GsViewRows* view_rows_host,
                                 int32_t dims, float* out, void* stream) {
  GS_REQUIRE(dims >= 1, GS_ERR_INVALID_ARGUMENT, "gs_views_sum_rows: dims %d", dims);
  GS_REQUIRE(dims <= (1 << 20), GS_ERR_UNSUPPORTED, "gs_views_sum_rows: rows of %d floats (at most %d)", dims, 1 << 20);
  GS_REQUIRE(rows >= 0 && rows < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT, "gs_views_sum_rows: %lld rows",
             (long long)rows);
  GS_REQUIRE(views >= 0 && views <= GS_VIEWS_MAX, GS_ERR_INVALID_ARGUMENT, "gs_views_sum_rows: views %d not in [0,%d]",
             views, GS_VIEWS_MAX);
  if (rows == 0) return GS_OK;
  GS_REQUIRE(indexes && out && (views == 0 || view_rows_host), GS_ERR_INVALID_ARGUMENT,
             "gs_views_sum_rows: NULL buffer");
  ViewsArgs a{};
  a.rows = rows; a.indexes = indexes; a.dims = dims; a.out = out;
  bool v4 = dims % 4 == 0 && aligned16(out);
  for (int b = 0; b < views; ++b) {  // a view without value rows adds nothing: it is left out, the order of the rest kept
    const GsViewRows& v = view_rows_host[b];
    GS_REQUIRE(v.count >= 0 && v.count < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT,
               "gs_views_sum_rows: view %d has %lld value rows", b, (long long)v.count);
    if (v.count == 0) continue;
    GS_REQUIRE(v.slot_of && v.values, GS_ERR_INVALID_ARGUMENT, "gs_views_sum_rows: NULL buffer (view %d)", b);
    GS_REQUIRE(v.stride >= dims, GS_ERR_INVALID_ARGUMENT, "gs_views_sum_rows: view %d has a stride of %d for %d floats",
               b, v.stride, dims);
    const int k = a.views++;
    a.slot_of[k] = v.slot_of; a.values[k] = v.values; a.count[k] = int32_t(v.count); a.stride[k] = v.stride;
    v4 = v4 && v.stride % 4 == 0 && aligned16(v.values);
  }
  if (v4)
    for (int k = 0; k < a.views; ++k) a.stride[k] /= 4;  // in 16-byte pieces
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 lanes(unsigned(gs_div_up(rows, kThreads)));
  if (dims == 1) hipLaunchKernelGGL((views_sum_narrow_kernel<1, false>), lanes, dim3(kThreads), 0, s, a);
  else if (dims == 2) hipLaunchKernelGGL((views_sum_narrow_kernel<2, false>), lanes, dim3(kThreads), 0, s, a);
  else if (dims == 3) hipLaunchKernelGGL((views_sum_narrow_kernel<3, false>), lanes, dim3(kThreads), 0, s, a);
  else if (dims == 4 && v4) hipLaunchKernelGGL((views_sum_narrow_kernel<4, true>), lanes, dim3(kThreads), 0, s, a);
  else if (dims == 4) hipLaunchKernelGGL((views_sum_narrow_kernel<4, false>), lanes, dim3(kThreads), 0, s, a);
  else if (v4) launch_views_wide_lanes<4>(a, s);
  else launch_views_wide_lanes<1>(a, s);
  GS_CHECK_LAUNCH("gs_views_sum_rows");
  return GS_OK;
}
