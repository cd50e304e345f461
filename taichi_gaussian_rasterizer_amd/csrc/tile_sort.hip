// tile_sort.hip -- everything that sorts: the per-tile depth sort behind gs_map_finish (one wave per tile: bucket sort,
// else rank sort; a workgroup per crowded tile: merge sort in LDS, else the bitonic network in global memory) with the
// launch ladder that picks between them, and gs_segmented_sort_pairs on the same machinery.
//
// A tile's bucket holds 64-bit composites (depth key << 32 | Gaussian index, written by mapper.hip's bucket pass).  They
// are unique, so the ascending order is independent of the order the bucket was filled in and equal to the reference's
// stable radix sort of (tile << 32 | depth) in generation order.  HBM traffic: K*8 B read + K*4 B written.
//
// Compiled with the mapper's flags (-ffp-contract=off): the one f32 multiply here (the bucket sort's digit) feeds no
// add, so the flag changes nothing; it is kept so that the mapper's units are built alike.

#include "map_query.h"

namespace {

// The one place the sorted layout is produced: the Gaussian index (low word of the composite) -> overlap_to_point, and
// the key map_to_tiles(return_keys=True) promises: the depth key under the tile id (tile << 32 | depth, or << 16).
__device__ __forceinline__ void store_sorted(uint64_t kv, int pos, int tile, int shift, int* o2p, uint64_t* keys_out) {
  o2p[pos] = int(uint32_t(kv));
  if (keys_out) keys_out[pos] = (kv >> 32) | (uint64_t(uint32_t(tile)) << shift);
}

// One workgroup per tile.  n <= CAP: bitonic sort in LDS.  n > CAP: the same network in place in
// global memory (rare: more than CAP splats on one tile); a workgroup lives on one CU, so its own
// global writes are visible to it after __syncthreads().
// The network is the direction-free bitonic formulation: each merge of width k starts with a
// mirror step (partner i ^ (k-1)) and continues with partners i ^ j, j = k/4 .. 1; every
// compare-exchange puts the minimum at the lower index.  Elements at index >= n are virtual +inf:
// they never move, so no padding is stored and n need not be a power of two.
template <int THREADS>
__device__ __forceinline__ void bitonic_sort(uint64_t* data, int n, int t) {
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int k = 2; k <= np2; k <<= 1) {
    for (int i = t; i < n; i += THREADS) {
      const int l = i ^ (k - 1);
      if (l > i && l < n) {
        const uint64_t x = data[i], y = data[l];
        if (x > y) { data[i] = y; data[l] = x; }
      }
    }
    __syncthreads();
    for (int j = k >> 2; j > 0; j >>= 1) {
      for (int i = t; i < n; i += THREADS) {
        const int l = i ^ j;
        if (l > i && l < n) {
          const uint64_t x = data[i], y = data[l];
          if (x > y) { data[i] = y; data[l] = x; }
        }
      }
      __syncthreads();
    }
  }
}

// Two-level rank sort of R rows of 64 keys by one wave (lane l holds mine[q] = rows[q * 64 + l]; keys are unique):
//   1. every row is ranked against ITSELF: 64 wave-uniform LDS broadcasts per row, lanes count (n compares per lane
//      instead of n*R), and the row is written back to LDS in sorted order, in place: every broadcast is done by then;
//   2. `fence` makes the wave's own row writes visible to its lanes; a key's rank among the other rows is a lower bound
//      in each of those sorted rows: 7 probes.
// rank[q] = final position of mine[q] among the R * 64 keys.  No data-dependent control flow.
template <int R, typename Fence>
__device__ __forceinline__ void rank_rows(uint64_t* rows, int lane, uint64_t (&mine)[R], int (&rank)[R], Fence fence) {
#pragma unroll
  for (int q = 0; q < R; ++q) { mine[q] = rows[q * 64 + lane]; rank[q] = 0; }
  for (int j = 0; j < 64; ++j) {
#pragma unroll
    for (int q = 0; q < R; ++q) rank[q] += rows[q * 64 + j] < mine[q] ? 1 : 0;
  }
#pragma unroll
  for (int q = 0; q < R; ++q) rows[q * 64 + rank[q]] = mine[q];
  fence();
#pragma unroll
  for (int q = 0; q < R; ++q) {
#pragma unroll
    for (int p = 0; p < R; ++p) {
      if (p == q) continue;
      const uint64_t* row = rows + p * 64;
      int pos = 0;
#pragma unroll
      for (int step = 32; step >= 1; step >>= 1) pos += row[pos + step - 1] < mine[q] ? step : 0;
      pos += row[pos] < mine[q] ? 1 : 0;
      rank[q] += pos;
    }
  }
}

// Merge sort of one crowded bucket (n <= CAP keys) in LDS by a whole workgroup.  Chunks of 256 are sorted by one
// wave each the way the wave rank sort does it; then runs are merged pairwise, each key finding its place by a
// lower bound in the partner run (keys are unique), ping-pong between two LDS buffers: log2(n / 256) barriers,
// against 78 for the bitonic network at 4096 keys.
template <int THREADS, int CAP>
__device__ __forceinline__ uint64_t* lds_merge_sort(uint64_t* a, uint64_t* b, int n, int t) {
  const int np = (n + 255) & ~255;  // pad to whole chunks with unique keys above every real one
  for (int i = n + t; i < np; i += THREADS) a[i] = 0xFFFFFFFF00000000ull | uint64_t(i);
  __syncthreads();
  // chunks of 256: one wave each, the two-level rank sort the wave kernel uses (rank_rows<4>), a -> b.  Only the wave's
  // own chunk is touched, so no workgroup barrier.
  const int lane = t & 63;
  for (int base = (t >> 6) * 256; base < np; base += (THREADS >> 6) * 256) {
    uint64_t mine[4];
    int rank[4];
    // the wave's own LDS writes, before its lanes read them
    rank_rows<4>(a + base, lane, mine, rank, [] { __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); });
#pragma unroll
    for (int q = 0; q < 4; ++q) b[base + rank[q]] = mine[q];
  }
  __syncthreads();
  uint64_t* src = b;
  uint64_t* dst = a;
  for (int width = 256; width < np; width <<= 1) {
    for (int i = t; i < np; i += THREADS) {
      const uint64_t mine = src[i];
      const int run = i / width, pos = i - run * width;
      const int pstart = (run ^ 1) * width;
      const int plen = max(0, min(width, np - pstart));
      const uint64_t* partner = src + pstart;
      int lo = 0, hi = plen;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (partner[mid] < mine) lo = mid + 1; else hi = mid;
      }
      dst[(run & ~1) * width + pos + lo] = mine;
    }
    __syncthreads();
    uint64_t* tmp = src; src = dst; dst = tmp;
  }
  return src;
}

// Catch-all for buckets fuller than the wave rank sort covers (n > min_n), grid-stride over the tiles (almost
// every tile is skipped).  n <= CAP: merge sort in LDS.  Beyond: the bitonic network in place in global memory.
template <int THREADS, int CAP>
__global__ __launch_bounds__(THREADS) void tile_sort_kernel(int num_tiles, const int2* tile_ranges, uint64_t* pairs,
                                                            int* o2p, uint64_t* keys_out, int depth16, int min_n,
                                                            int max_n) {
  extern __shared__ uint64_t s_sort[];  // 2 * CAP keys (dynamic: 128 KB of the CU's 160 KB at CAP = 8192)
  uint64_t* s_a = s_sort;
  uint64_t* s_b = s_sort + CAP;
  for (int tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
    const int2 r = tile_ranges[tile];
    const int n = r.y - r.x;
    if (n <= min_n || n > max_n) continue;  // uniform over the workgroup; another launch covers the rest
    uint64_t* seg = pairs + r.x;
    const int t = threadIdx.x;
    const uint64_t* data = seg;
    if (n <= CAP) {
      for (int i = t; i < n; i += THREADS) s_a[i] = seg[i];
      data = lds_merge_sort<THREADS, CAP>(s_a, s_b, n, t);  // starts with a barrier
    } else {
      __syncthreads();
      bitonic_sort<THREADS>(seg, n, t);
    }
    const int shift = depth16 ? 16 : 32;
    for (int i = t; i < n; i += THREADS) {
      store_sorted(data[i], r.x + i, tile, shift, o2p, keys_out);
    }
    __syncthreads();
  }
}

// cuda_lib.segmented_sort_pairs (cuda_lib/segmented_sort_pairs.cu:8-78): ascending sort of (key, value) pairs inside
// each [start, end) segment; signed 16- or 32-bit keys, int32 values.  One workgroup per segment (grid-stride) on the
// same machinery as the crowded-tile sort: composites (biased key << 32 | position in the segment) are unique, so the
// result is the stable order.
template <typename K, int THREADS, int CAP>
__global__ __launch_bounds__(THREADS) void segmented_sort_kernel(int num_segments, const int64_t* seg_start,
                                                                 const int64_t* seg_end, const K* keys,
                                                                 const int* values, K* keys_out, int* values_out,
                                                                 uint64_t* scratch) {
  extern __shared__ uint64_t s_sort[];
  uint64_t* s_a = s_sort;
  uint64_t* s_b = s_sort + CAP;
  const int t = threadIdx.x;
  const uint32_t bias = sizeof(K) == 2 ? 0x8000u : 0x80000000u;  // signed -> unsigned order
  for (int seg = blockIdx.x; seg < num_segments; seg += gridDim.x) {
    const int64_t lo = seg_start[seg];
    const int n = int(seg_end[seg] - lo);
    if (n <= 0) continue;
    uint64_t* stage = n <= CAP ? s_a : scratch + lo;
    for (int i = t; i < n; i += THREADS) {
      const uint32_t k = (sizeof(K) == 2 ? uint32_t(uint16_t(keys[lo + i])) : uint32_t(keys[lo + i])) ^ bias;
      stage[i] = (uint64_t(k) << 32) | uint64_t(uint32_t(i));
    }
    const uint64_t* data;
    if (n <= CAP) {
      data = lds_merge_sort<THREADS, CAP>(s_a, s_b, n, t);
    } else {
      __syncthreads();
      bitonic_sort<THREADS>(stage, n, t);
      data = stage;
    }
    for (int i = t; i < n; i += THREADS) {
      const uint64_t kv = data[i];
      keys_out[lo + i] = K(uint32_t(kv >> 32) ^ bias);
      values_out[lo + i] = values[lo + int(uint32_t(kv))];
    }
    __syncthreads();
  }
}

// Rank sort, one WAVE per tile, for buckets of up to 64*R pairs (the common case: a few hundred
// splats per tile).  Keys are unique (the Gaussian index is the low word), so the rank of a key
// -- the number of keys below it -- is its final position.  Each lane keeps R keys in registers
// (row q = keys q*64 .. q*64+63) and ranks them in two levels (rank_rows above; one row: against the bucket itself).
// A workgroup is one wave, so the barrier between the levels is only the wave's fence.  Slots past n hold pad keys
// 0xFFFFFFFF'00000000 | slot: unique, above every real key (the high word of a real key is the bit
// pattern of a depth in [0,1] or a 16-bit code), so they sort to the end of their row.
template <int R>
__device__ __forceinline__ void rank_sort_rows(uint64_t* s_key, int n, int lane, int start, int tile, int* o2p,
                                               uint64_t* keys_out, int shift) {
  uint64_t mine[R];
  int rank[R];
  if (R == 1) {
    mine[0] = s_key[lane];
    rank[0] = 0;
    for (int j = 0; j < n; ++j) rank[0] += s_key[j] < mine[0] ? 1 : 0;
  } else {
    rank_rows<R>(s_key, lane, mine, rank, [] { __syncthreads(); });
  }
#pragma unroll
  for (int q = 0; q < R; ++q) {
    if ((mine[q] >> 32) != 0xFFFFFFFFull) store_sorted(mine[q], start + rank[q], tile, shift, o2p, keys_out);
  }
}

// Bucket sort of the same buckets, tried first (round 3): depths inside a tile are spread out, so a counting sort on
// a 256-bin digit of the depth word leaves ~1 key per bin and a key's final position is its bin's start plus its rank
// among the handful of keys that share the bin -- ~10 + 2 (keys per bin) compares per key instead of 64 broadcast
// compares per row and key plus 7 probes for every other row.  The digit is floor((depth word - min) * 256 / (max -
// min + 1)) in f32: monotonic in the depth word, which is all the final order needs (ties inside a bin are resolved on
// the full 64-bit composite).  Keys are scattered IN PLACE (s_key is dead once every lane holds its rows in registers).
// Returns false, leaving the registers' worth of keys unplaced, when some bin holds more than BIN_LIMIT keys (depths
// clustered on one surface): the caller reloads the bucket and runs the rank sort above, whose cost does not depend
// on the distribution.
#ifndef GS_SORT_BINS
#define GS_SORT_BINS 1
#endif
constexpr int SORT_BINS = 256, BIN_LIMIT = 40;

template <int R>
__device__ __forceinline__ bool bucket_sort_rows(uint64_t* s_key, int* s_hist, int n, int lane, int start, int tile,
                                                 int* o2p, uint64_t* keys_out, int shift) {
  uint64_t mine[R];
  uint32_t mn = 0xFFFFFFFFu, mx = 0u;
#pragma unroll
  for (int q = 0; q < R; ++q) {
    mine[q] = s_key[q * 64 + lane];
    if (q * 64 + lane < n) {
      const uint32_t hi = uint32_t(mine[q] >> 32);
      mn = min(mn, hi);
      mx = max(mx, hi);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mn = min(mn, uint32_t(__shfl_xor(int(mn), off)));
    mx = max(mx, uint32_t(__shfl_xor(int(mx), off)));
  }
  const float scale = float(SORT_BINS) / (float(mx - mn) + 1.0f);
#pragma unroll
  for (int k = 0; k < SORT_BINS / 64; ++k) s_hist[k * 64 + lane] = 0;
  __syncthreads();
  int bin[R], arrival[R];
#pragma unroll
  for (int q = 0; q < R; ++q) {
    bin[q] = 0; arrival[q] = 0;
    if (q * 64 + lane < n) {
      bin[q] = min(SORT_BINS - 1, int(float(uint32_t(mine[q] >> 32) - mn) * scale));
      arrival[q] = atomicAdd(&s_hist[bin[q]], 1);
    }
  }
  __syncthreads();
  // exclusive scan of the bins: lane l owns bins 4 l .. 4 l + 3
  int c[SORT_BINS / 64], local = 0, fullest = 0;
#pragma unroll
  for (int k = 0; k < SORT_BINS / 64; ++k) {
    c[k] = s_hist[lane * (SORT_BINS / 64) + k];
    local += c[k];
    fullest = max(fullest, c[k]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) fullest = max(fullest, __shfl_xor(fullest, off));
  if (fullest > BIN_LIMIT) return false;  // wave-uniform
  int run = wave_inclusive_scan(local) - local;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SORT_BINS / 64; ++k) {
    s_hist[lane * (SORT_BINS / 64) + k] = run;
    run += c[k];
  }
  if (lane == 63) s_hist[SORT_BINS] = run;  // = n
  __syncthreads();
#pragma unroll
  for (int q = 0; q < R; ++q)
    if (q * 64 + lane < n) s_key[s_hist[bin[q]] + arrival[q]] = mine[q];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < R; ++q) {
    if (q * 64 + lane >= n) continue;
    const int b0 = s_hist[bin[q]], b1 = s_hist[bin[q] + 1];
    int rank = b0;
    for (int j = b0; j < b1; ++j) rank += s_key[j] < mine[q] ? 1 : 0;
    store_sorted(mine[q], start + rank, tile, shift, o2p, keys_out);
  }
  return true;
}

// RMAX bounds the LDS buffer (64*RMAX keys); the number of register rows is chosen PER TILE from its
// own population, so a 100-splat tile in a frame whose fullest tile holds 500 does 2 rows of
// compares, not 8.
template <int RMAX>
// __launch_bounds__(64, 6): left alone the compiler unrolls the 64 broadcast rounds with ~30 keys in flight and ends up
// at 195 VGPRs = 2 waves per SIMD for a kernel that waits on dependent LDS probes; asked for 6 waves per SIMD (<= 80
// VGPRs) the sort takes 37 us instead of 55 at C3 (measured: 3 / 4 / 6 / 8 waves -> 92 / 87 / 85 / 92 us for
// gs_map_finish).
__global__ __launch_bounds__(64, 6) void tile_rank_sort_kernel(int num_tiles, const int2* tile_ranges,
                                                            uint64_t* pairs, int* o2p, uint64_t* keys_out,
                                                            int depth16, int skip_full) {
  __shared__ uint64_t s_key[64 * RMAX];
  __shared__ int s_hist[SORT_BINS + 1];
  const int tile = gs_xcd_remap(blockIdx.x, num_tiles);
  if (tile < 0) return;
  const int2 r = tile_ranges[tile];
  const int n = r.y - r.x;
  if (n <= 0) return;
  const int lane = threadIdx.x;
  const int shift = depth16 ? 16 : 32;
  if (n > 64 * RMAX) {
    if (skip_full) return;  // a dedicated bitonic launch follows for these
    // fuller than this launch was sized for (only when the caller's hint was low): this wave sorts the
    // bucket in place in global memory -- slow, rare, and never wrong
    uint64_t* gseg = pairs + r.x;
    bitonic_sort<64>(gseg, n, lane);
    for (int i = lane; i < n; i += 64) store_sorted(gseg[i], r.x + i, tile, shift, o2p, keys_out);
    return;
  }
  const uint64_t* seg = pairs + r.x;
  const int rows = (n + 63) >> 6;  // exactly as many register rows as the bucket needs (cost grows with rows^2)
  for (int i = lane; i < rows * 64; i += 64) s_key[i] = i < n ? seg[i] : (0xFFFFFFFF00000000ull | uint64_t(i));
  __syncthreads();
  if (GS_SORT_BINS && rows >= 2) {
    bool done = false;
    switch (rows) {
      case 2: done = bucket_sort_rows<2>(s_key, s_hist, n, lane, r.x, tile, o2p, keys_out, shift); break;
      case 3: done = bucket_sort_rows<3>(s_key, s_hist, n, lane, r.x, tile, o2p, keys_out, shift); break;
      case 4: done = bucket_sort_rows<4>(s_key, s_hist, n, lane, r.x, tile, o2p, keys_out, shift); break;
      case 5: done = bucket_sort_rows<(RMAX >= 8 ? 5 : 2)>(s_key, s_hist, n, lane, r.x, tile, o2p, keys_out, shift); break;
      case 6: done = bucket_sort_rows<(RMAX >= 8 ? 6 : 2)>(s_key, s_hist, n, lane, r.x, tile, o2p, keys_out, shift); break;
      case 7: done = bucket_sort_rows<(RMAX >= 8 ? 7 : 2)>(s_key, s_hist, n, lane, r.x, tile, o2p, keys_out, shift); break;
      default: done = bucket_sort_rows<(RMAX >= 8 ? 8 : 2)>(s_key, s_hist, n, lane, r.x, tile, o2p, keys_out, shift); break;
    }
    if (done) return;
    // clustered depths: s_key is untouched up to here (the scatter comes after the bin-size check)
  }
  switch (rows) {
    case 1: rank_sort_rows<1>(s_key, n, lane, r.x, tile, o2p, keys_out, shift); break;
    case 2: rank_sort_rows<2>(s_key, n, lane, r.x, tile, o2p, keys_out, shift); break;
    case 3: rank_sort_rows<3>(s_key, n, lane, r.x, tile, o2p, keys_out, shift); break;
    case 4: rank_sort_rows<4>(s_key, n, lane, r.x, tile, o2p, keys_out, shift); break;
    case 5: rank_sort_rows<(RMAX >= 8 ? 5 : 1)>(s_key, n, lane, r.x, tile, o2p, keys_out, shift); break;
    case 6: rank_sort_rows<(RMAX >= 8 ? 6 : 1)>(s_key, n, lane, r.x, tile, o2p, keys_out, shift); break;
    case 7: rank_sort_rows<(RMAX >= 8 ? 7 : 1)>(s_key, n, lane, r.x, tile, o2p, keys_out, shift); break;
    default: rank_sort_rows<(RMAX >= 8 ? 8 : 1)>(s_key, n, lane, r.x, tile, o2p, keys_out, shift); break;
  }
}

}  // namespace

// The sort launches of gs_map_finish, chosen from the population of the fullest tile.
int gs_map_sort_tiles(int num_tiles, const int32_t* tile_ranges, uint64_t* pairs, int32_t* overlap_to_point,
                      uint64_t* sorted_keys, int32_t use_depth16, int32_t max_tile_count, hipStream_t s) {
  const int grid = 8 * int(gs_div_up(num_tiles, 8));
  const int2* r = reinterpret_cast<const int2*>(tile_ranges);
  // max_tile_count > 0: exact population of the fullest tile (read back by the caller);
  // max_tile_count <= 0: unknown -- |max_tile_count| is a hint (0 = none).  A wrong hint costs time only.
  const bool exact = max_tile_count > 0;
  const int guess = exact ? max_tile_count : (max_tile_count < 0 ? -max_tile_count : 1024);
  // Wave rank sort for buckets of up to 256 / 512 pairs (4 KB of LDS per wave at most, so a few crowded tiles
  // do not cost every tile its occupancy); fuller buckets go to the workgroup-per-tile launch when such tiles
  // are known or expected, otherwise (a hint that turns out low) the rank-sort wave sorts them itself, slowly.
  const bool big_pass = guess > 512;
  const int skip_full = (exact || big_pass) ? 1 : 0;
  int covered;
  if (guess <= 256) {
    covered = 256;
    hipLaunchKernelGGL((tile_rank_sort_kernel<4>), dim3(grid), dim3(64), 0, s, num_tiles, r, pairs, overlap_to_point,
                       sorted_keys, use_depth16, skip_full);
  } else {
    covered = 512;
    hipLaunchKernelGGL((tile_rank_sort_kernel<8>), dim3(grid), dim3(64), 0, s, num_tiles, r, pairs, overlap_to_point,
                       sorted_keys, use_depth16, skip_full);
  }
  if (big_pass) {
    // 513 .. 1024 and 1025 .. 2048 pairs: 256-thread workgroups with 16 / 32 KB of LDS (ten / five per CU -- in dense
    // scenes most tiles are here); above that: 1024 threads and 128 KB (one per CU).  A size class is launched only
    // when such tiles are expected.
    constexpr int SMALL = 1024, MID = 2048, CAP = 8192;
    const bool mid_pass = guess > SMALL, huge_pass = guess > MID;
    static const hipError_t lds_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&tile_sort_kernel<1024, CAP>),
                                                          hipFuncAttributeMaxDynamicSharedMemorySize, 2 * CAP * 8);
    GS_REQUIRE(lds_ok == hipSuccess, GS_ERR_LAUNCH, "gs_map_finish: cannot reserve %d bytes of LDS", 2 * CAP * 8);
    // each launch takes the sizes the later ones do not cover (the last one launched takes everything above)
    hipLaunchKernelGGL((tile_sort_kernel<256, SMALL>), dim3(min(num_tiles, 8192)), dim3(256), 2 * SMALL * 8, s,
                       num_tiles, r, pairs, overlap_to_point, sorted_keys, use_depth16, covered,
                       mid_pass ? SMALL : 0x7fffffff);
    if (mid_pass)
      hipLaunchKernelGGL((tile_sort_kernel<256, MID>), dim3(min(num_tiles, 8192)), dim3(256), 2 * MID * 8, s,
                         num_tiles, r, pairs, overlap_to_point, sorted_keys, use_depth16, SMALL,
                         huge_pass ? MID : 0x7fffffff);
    if (huge_pass)
      hipLaunchKernelGGL((tile_sort_kernel<1024, CAP>), dim3(min(num_tiles, 2048)), dim3(1024), 2 * CAP * 8, s,
                         num_tiles, r, pairs, overlap_to_point, sorted_keys, use_depth16, MID, 0x7fffffff);
  }
  GS_CHECK_LAUNCH("gs_map_finish/sort");
  return GS_OK;
}

extern "C" int gs_segmented_sort_pairs(int64_t num_items, int32_t key_bytes, const void* keys, const int32_t* values,
                                       void* keys_out, int32_t* values_out, int64_t num_segments,
                                       const int64_t* start_offsets, const int64_t* end_offsets, void* scratch,
                                       int64_t scratch_bytes, void* stream) {
  GS_REQUIRE(key_bytes == 2 || key_bytes == 4, GS_ERR_UNSUPPORTED,
             "gs_segmented_sort_pairs: %d-byte keys (int16 and int32 are implemented, as in the reference)", key_bytes);
  GS_REQUIRE(num_items >= 0 && num_items < (int64_t(1) << 31) && num_segments >= 0, GS_ERR_INVALID_ARGUMENT,
             "gs_segmented_sort_pairs: %lld items, %lld segments", (long long)num_items, (long long)num_segments);
  if (num_items == 0 || num_segments == 0) return GS_OK;
  GS_REQUIRE(keys && values && keys_out && values_out && start_offsets && end_offsets, GS_ERR_INVALID_ARGUMENT,
             "gs_segmented_sort_pairs: NULL buffer");
  GS_REQUIRE(scratch && scratch_bytes >= num_items * 8, GS_ERR_SCRATCH_TOO_SMALL,
             "gs_segmented_sort_pairs: scratch %lld < %lld bytes", (long long)scratch_bytes, (long long)num_items * 8);
  constexpr int CAP = 8192;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(unsigned(num_segments < 4096 ? num_segments : 4096));
  if (key_bytes == 4) {
    static const hipError_t ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&segmented_sort_kernel<int32_t, 1024, CAP>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, 2 * CAP * 8);
    GS_REQUIRE(ok == hipSuccess, GS_ERR_LAUNCH, "gs_segmented_sort_pairs: cannot reserve LDS");
    hipLaunchKernelGGL((segmented_sort_kernel<int32_t, 1024, CAP>), grid, dim3(1024), 2 * CAP * 8, s, int(num_segments),
                       start_offsets, end_offsets, static_cast<const int32_t*>(keys), values,
                       static_cast<int32_t*>(keys_out), values_out, static_cast<uint64_t*>(scratch));
  } else {
    static const hipError_t ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&segmented_sort_kernel<int16_t, 1024, CAP>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, 2 * CAP * 8);
    GS_REQUIRE(ok == hipSuccess, GS_ERR_LAUNCH, "gs_segmented_sort_pairs: cannot reserve LDS");
    hipLaunchKernelGGL((segmented_sort_kernel<int16_t, 1024, CAP>), grid, dim3(1024), 2 * CAP * 8, s, int(num_segments),
                       start_offsets, end_offsets, static_cast<const int16_t*>(keys), values,
                       static_cast<int16_t*>(keys_out), values_out, static_cast<uint64_t*>(scratch));
  }
  GS_CHECK_LAUNCH("gs_segmented_sort_pairs");
  return GS_OK;
}
