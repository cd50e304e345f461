// mapper.hip -- tile-overlap cull and per-tile bucketing: the fused path of the tile mapper
// (reference mapper/tile_mapper.py:74-196, taichi_lib/grid_query.py:10-91).  The query and its bit-exactness contract
// (-ffp-contract=off, gs_det_sqrtf / gs_det_logf, the oracle's op order) are map_query.h's; the per-tile sorts are
// tile_sort.hip's; the reference-shaped primitives that cross-check this path are map_reference.hip's.
//
// Fused path (gs_map_prepare / gs_map_finish), designed for MI355X rather than around a
// library radix sort:
//   bin     : order the Gaussians by the screen region (8x8 tiles; larger when the image has more than
//             1024 of them) of their centre -- LDS histograms per workgroup of 1024 Gaussians, then either one
//             returning atomic per (workgroup, region) (small frames: no launch of its own) or a per-region scan
//             over the workgroups (large frames), and a scatter.  In the frame calls the histogram pass IS the
//             projection's compaction pass (compact_bin_kernel).
//   count   : 1 lane per Gaussian, OBB query; overlaps are counted in an LDS window over the
//             workgroup's region (+ border) and flushed with one atomic per window tile into a T-entry
//             histogram (scattered 4-B global atomics only reach ~20 G/s on MI355X).
//   scan    : single workgroup exclusive scan of the histogram -> tile_ranges, cursors, K, max, and the
//             rasterizer's launch order (tiles by descending population).
//   emit    : the query again; one returning atomic per (workgroup, tile) reserves a range of the
//             tile's bucket, LDS atomics place the 64-bit composites (depth key << 32 | index).
//   sort    : tile_sort.hip (gs_map_sort_tiles): one wave per tile sorts its bucket.
// HBM traffic: K*8 B written by emit, K*8 B read + K*4 B written by sort, against
// 6 passes * 2 * 12 B * K for the reference's Onesweep sort (profiles/bicycle_2048.txt:7).

#include "map_query.h"

namespace {

// One workgroup: exclusive scan of the T-entry tile histogram (coalesced rounds of 1024 tiles) ->
// tile_ranges, bucket cursors, K, fullest tile, overflow flag; beside it a second workgroup builds the rasterizer's
// launch order: tiles by descending population (counting sort on min(count, 1023); the order inside a
// bin comes from LDS atomics and is arbitrary -- it only affects scheduling).
__global__ __launch_bounds__(1024) void map_scan_kernel(int num_tiles, const int* tile_hist, int2* tile_ranges,
                                                        int* cursors, int* counts_out, int64_t k_capacity,
                                                        int* tile_order, const int* v_dev, int* counts_host,
                                                        const int* touched_dev) {
  // workgroup 0: tile ranges, cursors, K / fullest tile / overflow; workgroup 1 (launched only with a tile_order):
  // the launch order and the heavy-tile count.  Both read the same histogram and neither waits for the other.
  __shared__ int s_wave[16];
  __shared__ int s_bin[1024];
  const int t = threadIdx.x;
  if (blockIdx.x == 0) {
    // Round 3: every thread owns PER consecutive tiles of a round (64 bytes: four 16-byte loads), scans them serially
    // in registers and takes part in ONE workgroup scan of the per-thread totals per 16 384 tiles -- two barriers per
    // round instead of the 32 of a scan per 1024 tiles (14.5 -> ~5 us at 16 384 tiles).  Ranges and cursors leave as
    // 16-byte stores.
    constexpr int PER = 16;
    int carry = 0, mx = 0;
    for (int base0 = 0; base0 < num_tiles; base0 += 1024 * PER) {
      const int i0 = base0 + t * PER;
      int c[PER];
      const bool whole = i0 + PER <= num_tiles;
      if (whole) {
        const int4* src = reinterpret_cast<const int4*>(tile_hist + i0);
#pragma unroll
        for (int q = 0; q < PER / 4; ++q) {
          const int4 v4 = src[q];
          c[4 * q] = v4.x; c[4 * q + 1] = v4.y; c[4 * q + 2] = v4.z; c[4 * q + 3] = v4.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < PER; ++j) c[j] = i0 + j < num_tiles ? tile_hist[i0 + j] : 0;
      }
      int sum = 0;
#pragma unroll
      for (int j = 0; j < PER; ++j) { sum += c[j]; mx = max(mx, c[j]); }
      int total;
      int run = carry + block_exclusive_scan(sum, s_wave, total);
      carry += total;
      int2 rg[PER];
      int cur[PER];
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        // a tile that would run past the caller's pair capacity is dropped (and flagged below): the
        // caller re-runs with a larger buffer; nothing downstream may index past k_capacity
        const bool fits = k_capacity <= 0 || int64_t(run) + c[j] <= k_capacity;
        rg[j] = (c[j] > 0 && fits) ? make_int2(run, run + c[j]) : make_int2(0, 0);  // tile_mapper.py:186
        cur[j] = fits ? run : -(1 << 30);  // negative for the whole launch: any returning add reports it
        run += c[j];
      }
      if (whole) {
        int4* dr = reinterpret_cast<int4*>(tile_ranges + i0);
        int4* dc = reinterpret_cast<int4*>(cursors + i0);
#pragma unroll
        for (int q = 0; q < PER / 2; ++q) dr[q] = make_int4(rg[2 * q].x, rg[2 * q].y, rg[2 * q + 1].x, rg[2 * q + 1].y);
#pragma unroll
        for (int q = 0; q < PER / 4; ++q) dc[q] = make_int4(cur[4 * q], cur[4 * q + 1], cur[4 * q + 2], cur[4 * q + 3]);
      } else {
#pragma unroll
        for (int j = 0; j < PER; ++j)
          if (i0 + j < num_tiles) { tile_ranges[i0 + j] = rg[j]; cursors[i0 + j] = cur[j]; }
      }
    }
    // fullest tile
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, __shfl_xor(mx, off));
    if ((t & 63) == 0) s_wave[t >> 6] = mx;
    __syncthreads();
    if (t == 0) {
      int m = 0;
      for (int w = 0; w < 16; ++w) m = max(m, s_wave[w]);
      const int over = (k_capacity > 0 && int64_t(carry) > k_capacity) ? 1 : 0;
      counts_out[0] = carry;
      counts_out[1] = m;
      counts_out[2] = over;
      if (!tile_order) counts_out[3] = 0;
      if (counts_host) {  // pinned host words, visible to the host once this kernel has completed: no copy launch
        counts_host[0] = carry;
        counts_host[1] = m;
        counts_host[2] = over;
        if (!tile_order) counts_host[3] = 0;
        counts_host[4] = v_dev ? *v_dev : 0;
        counts_host[5] = touched_dev ? *touched_dev : 0;  // Gaussians in the region order = splats that can reach an owned row
      }
    }
    return;
  }
  // ---- workgroup 1: counting sort of the tiles by descending overlap count (1024 bins, the last one open-ended).
  // One pass over the histogram: a thread keeps its PER consecutive counts of a round in registers between the
  // binning and the scatter (rounds beyond the first -- more than 16 384 tiles -- read the histogram twice).
  constexpr int PER = 16;
  s_bin[t] = 0;
  __syncthreads();
  int sum = 0;
  int c0[PER];
  for (int base0 = 0; base0 < num_tiles; base0 += 1024 * PER) {
    const int i0 = base0 + t * PER;
    int c[PER];
    if (i0 + PER <= num_tiles) {
      const int4* src = reinterpret_cast<const int4*>(tile_hist + i0);
#pragma unroll
      for (int q = 0; q < PER / 4; ++q) {
        const int4 v4 = src[q];
        c[4 * q] = v4.x; c[4 * q + 1] = v4.y; c[4 * q + 2] = v4.z; c[4 * q + 3] = v4.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < PER; ++j) c[j] = i0 + j < num_tiles ? tile_hist[i0 + j] : -1;
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (base0 == 0) c0[j] = c[j];
      if (c[j] >= 0) {
        sum += c[j];
        atomicAdd(&s_bin[min(c[j], 1023)], 1);
      }
    }
  }
  int unused, k_total;
  block_exclusive_scan(sum, s_wave, k_total);
  // start of bin b in descending order = number of tiles in fuller bins: scan the bins from the top
  const int start = block_exclusive_scan(s_bin[1023 - t], s_wave, unused);
  s_bin[1023 - t] = start;  // read above and written here by the same thread only
  // counts_out[3] = number of "heavy" tiles at the head of the order, which the rasterizer splits into four
  // 8x8 workgroups each.  A launch cannot end before ONE wave has walked its fullest tile (n splats take about
  // 1.75 n c when the wave has a SIMD to itself), while the whole launch takes about K c / 1024 on 1024 SIMDs:
  // tiles with n > K / 1792 are the ones that bound it.  Large grids (K / 1792 above every tile) split nothing.
  {
    const int thr_bin = min(max(k_total / 1792, 96), 1022);
    if (1023 - t == thr_bin) {
      const int heavy = min(start, num_tiles / 4);  // tiles in bins above thr_bin
      counts_out[3] = heavy;
      if (counts_host) counts_host[3] = heavy;
    }
  }
  __syncthreads();
  for (int base0 = 0; base0 < num_tiles; base0 += 1024 * PER) {
    const int i0 = base0 + t * PER;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int c = base0 == 0 ? c0[j] : (i0 + j < num_tiles ? tile_hist[i0 + j] : -1);
      if (c >= 0 && i0 + j < num_tiles) tile_order[atomicAdd(&s_bin[min(c, 1023)], 1)] = i0 + j;
    }
  }
}

// ---- region-binned counting / bucketing --------------------------------------------------
// Scattered 4-byte global atomics run at only ~20 G/s on MI355X (every one is its own 64-B
// memory-side request), which made the plain count / emit kernels above atomic-bound (K atomics
// each).  The binned path first orders the Gaussians by the screen REGION of their centre, then lets
// every workgroup -- whose CHUNK Gaussians now share one region -- count its overlaps in an LDS window
// covering the region plus a border, and touch global memory once per window tile.
// The region edge is the smallest power of two >= RG_MIN that keeps the region count <= MAX_REGIONS: the
// smaller the region, the more of a workgroup's overlaps share a window tile, i.e. the fewer global atomics
// (8x8-tile regions: ~5 overlaps per atomic at 256 Gaussians per workgroup; 32x32: ~1.4).
constexpr int RG_MIN = 8;              // smallest region edge in tiles
constexpr int RB = 4;                  // window border in tiles (splats reaching further fall back to global atomics)
constexpr int MAX_REGIONS = 1024;
constexpr int WIDE_SPAN = 64;          // candidate tiles above which a splat is walked by its whole wave
#ifndef GS_MAP_CHUNK
#define GS_MAP_CHUNK 512
#endif
constexpr int CHUNK = GS_MAP_CHUNK;     // Gaussians (= threads) per counting / bucketing workgroup

struct RegionGrid {
  int tiles_x, tiles_y, regions_x, num_regions;
  int rg;    // region edge in tiles
  int win;   // window edge = rg + 2 RB; the LDS window holds win * win ints
  int row0;  // first tile row the grid covers (a contiguous shard's first row; 0 otherwise)
};

// Query cache (round 3): the counting pass leaves the outcome of its OBB query and per-tile tests as 16 bytes per
// Gaussian, in the REGION order it works in: the accepted tiles of the candidate span as a 64-bit mask (bit = ty *
// span_x + tx, owned rows only) and the span itself.  The bucketing pass, which walks the same order, reads those 16
// bytes sequentially instead of gathering the 28-byte row again and repeating the query and the tests (emit 48 -> 34 us
// at C3).  Spans above WIDE_SPAN tiles are flagged and walked by their whole wave from the row, as before.
// (Filling the cache in the binning pass instead, in index order, made that pass 23 us slower and the two consumers
// gather it at random: 7 us worse in all.)
struct QueryCache {
  unsigned long long accept;
  unsigned int x;  // min_tx (20 bits: up to 2^20 tiles) | span_x << 20
  unsigned int y;  // min_ty (20 bits) | span_y << 20 | wide << 31
};
constexpr unsigned QC_WIDE = 0x80000000u;
__device__ __forceinline__ int qc_min_tx(const QueryCache& q) { return int(q.x & 0xfffffu); }
__device__ __forceinline__ int qc_min_ty(const QueryCache& q) { return int(q.y & 0xfffffu); }
__device__ __forceinline__ int qc_span_x(const QueryCache& q) { return int((q.x >> 20) & 0x7fu); }

// The LDS window of a counting / bucketing workgroup: the tiles of its region plus RB on every side, laid out in
// full-image tile coordinates (rows the shard does not own stay zero).  The one place that says which tile has which
// window slot: the bucket pass's reservation per window tile is only right if its counting and placing passes and the
// flush between them agree on it.
struct Window {
  int x0, y0, win;
  __device__ __forceinline__ Window(const RegionGrid& rg, int region)
      : x0((region % rg.regions_x) * rg.rg - RB), y0((region / rg.regions_x) * rg.rg - RB + rg.row0), win(rg.win) {}
  // is tile (gx, gy) inside?  e = its window slot then.  (Not "slot or -1": the sign test on a value the compiler
  // cannot prove non-negative costs a v_cndmask and a v_cmp per tile in the counting and placing loops.)
  __device__ __forceinline__ bool slot(int gx, int gy, int& e) const {
    const int lx = gx - x0, ly = gy - y0;
    e = ly * win + lx;
    return unsigned(lx) < unsigned(win) && unsigned(ly) < unsigned(win);
  }
  __device__ __forceinline__ void tile_of(int e, int& gx, int& gy) const { gx = x0 + e % win; gy = y0 + e / win; }
};

// f(tx, ty) for every set bit of a lane's accept mask (bit = ty * span_x + tx over its candidate span)
template <typename F>
__device__ __forceinline__ void for_each_accepted(unsigned long long accept, int span_x, F f) {
  for (unsigned long long todo = accept; todo != 0ull; todo &= todo - 1ull) {
    const int bit = __ffsll(todo) - 1;
    const int ty = bit / span_x, tx = bit - ty * span_x;
    f(tx, ty);
  }
}

// Splats with a wide candidate span (hundreds of tiles for a floater that covers the screen) are walked by the whole
// wave, 64 tiles per step: one lane looping over them alone would hold its workgroup for milliseconds (a dependent
// global atomic per tile).  For every lane of `wide_lanes` in turn (its Gaussian index is that lane's i): the query
// again, then f(gi) once per splat gives the action g, and g(gx, gy) runs for every owned tile that passes the OBB test.
template <typename F>
__device__ __forceinline__ void for_each_wide_tile(const MapArgs& a, int i, uint64_t wide_lanes, F f) {
  for (uint64_t todo = wide_lanes; todo != 0ull; todo &= todo - 1ull) {
    const int gi = __shfl(i, __ffsll(static_cast<unsigned long long>(todo)) - 1);
    const GridQuery q = grid_query(a.points + 7 * int64_t(gi), a.Wp, a.Hp, a.tile_size, a.thr);
    auto g = f(gi);
    const int total = q.span_x * q.span_y;
    for (int k = int(threadIdx.x & 63); k < total; k += 64) {
      const int ty = k / q.span_x, tx = k - ty * q.span_x;
      if (gs_shard_owns(a.sh, ty + q.min_ty) && test_tile(q, tx, ty, a.tile_size)) g(tx + q.min_tx, ty + q.min_ty);
    }
  }
}

// Does the Gaussian enter the region order at all?  Leaving one out is only allowed when it has no tile here: the exact
// query decides for a sharded frame (most splats miss a rank's rows, and the sparse exchange lists exactly the ones that
// do not).  For a whole image nearly every visible Gaussian has a tile, and one that has none simply contributes
// nothing to the counting pass: the query is skipped (the answer may be conservative, never the other way round).
__device__ __forceinline__ bool enters_order(const float* g, const MapArgs& a) {
  if (a.sh.period == 1 && a.sh.begin == 0 && a.sh.end * a.tile_size >= a.Hp) return true;
  const GridQuery q = grid_query(g, a.Wp, a.Hp, a.tile_size, a.thr);
  return q.span_x > 0 && gs_shard_any_row(a.sh, q.min_ty, q.min_ty + q.span_y);
}

__device__ __forceinline__ int region_of_gaussian(const float* g, const MapArgs& a, const RegionGrid& rg) {
  const float ts = float(a.tile_size);
  int tx = int(floorf(g[0] / ts)), ty = int(floorf(g[1] / ts));
  tx = min(max(tx, 0), rg.tiles_x - 1);
  ty = min(max(ty - rg.row0, 0), rg.tiles_y - 1);  // the region grid starts at the shard's first row
  return (ty / rg.rg) * rg.regions_x + (tx / rg.rg);
}

// K1: per-workgroup region populations.  A workgroup reserves its place inside every region it holds Gaussians of with
// ONE returning atomic per (workgroup, region) on the region's counter and keeps the offset in part[region][workgroup]
// (round 3; ~250 atomics per workgroup of 1 024 Gaussians at C3, spread over 256 counters).  The order of the
// workgroups inside a region is the order their atomics arrive in -- it only decides which counting workgroup a
// Gaussian lands in, never a result: every tile's bucket is sorted on (depth, index) afterwards.  (Rounds 1 - 2 kept
// the order deterministic with two scan launches over the part matrix: 5 + 5 us at any size.)
// region_count must be zero when the pass starts (gs_map_bin_counters).
constexpr int BIN = 1024;
// region_count == nullptr: the scan launches follow (K2a / K2b); part[r][b] is the workgroup's own count
__device__ __forceinline__ void publish_region_hist(const int* s_hist, const RegionGrid& rg, int num_wg, int blk,
                                                    int* part, int* region_count) {
  for (int r = threadIdx.x; r < rg.num_regions; r += BIN) {
    const int h = s_hist[r];
    if (region_count == nullptr) part[int64_t(r) * num_wg + blk] = h;
    else if (h > 0) part[int64_t(r) * num_wg + blk] = atomicAdd(region_count + r, h);
  }
}

// K1's step for one row, and the bookkeeping of its workgroup (every thread of the workgroup calls it; `active`: the
// thread has a row g, whose region goes to *region_of_row).  A Gaussian whose candidate span is empty (off-screen
// within the cull margin; above or below this rank's strip when the frame is sharded) is left out of the ordering, so
// the counting and bucketing passes never see it.  (A non-empty span whose tiles all fail the OBB test is rare and
// simply contributes nothing.)  The rows of workgroup b are [block_start[b], block_start[b + 1]) = [first, first +
// rows) here; touched_blocks[b] says how many of them are in the ordering at all (gs_map_touched_list compacts them in
// ascending order).
__device__ __forceinline__ void bin_row(bool active, const float* g, const MapArgs& a, const RegionGrid& rg,
                                        int* region_of_row, int* s_hist, int first, int rows, int num_wg,
                                        int* touched_blocks, int* block_start) {
  bool binned = false;
  if (active) {
    const bool any = enters_order(g, a);
    const int r = any ? region_of_gaussian(g, a, rg) : -1;
    *region_of_row = r;
    if (r >= 0) atomicAdd(&s_hist[r], 1);
    binned = r >= 0;
  }
  const int touched = __syncthreads_count(binned);
  if (threadIdx.x == 0) {
    touched_blocks[blockIdx.x] = touched;
    block_start[blockIdx.x] = first;
    if (int(blockIdx.x) == num_wg - 1) block_start[num_wg] = first + rows;
  }
}

// The standalone binning pass: workgroup b holds rows b * BIN .. (compact_bin_kernel below: the ranges the projection's
// compaction pass produced when that pass did the binning itself).
__global__ __launch_bounds__(BIN) void region_count_kernel(MapArgs a, RegionGrid rg, int num_wg, int* region_of,
                                                           int* part, int* touched_blocks, int* block_start,
                                                           int* region_count) {
  __shared__ int s_hist[MAX_REGIONS];
  for (int r = threadIdx.x; r < rg.num_regions; r += BIN) s_hist[r] = 0;
  __syncthreads();
  const int64_t i = int64_t(blockIdx.x) * BIN + threadIdx.x;
  const int64_t live = live_count(a);
  const int first = int(min(int64_t(blockIdx.x) * BIN, live));
  bin_row(i < live, a.points + 7 * i, a, rg, region_of + i, s_hist, first, int(live) - first, num_wg, touched_blocks,
          block_start);
  publish_region_hist(s_hist, rg, num_wg, blockIdx.x, part, region_count);
}

// Two ways from the per-workgroup histograms to "where does workgroup b start inside region r" (part[r][b]), chosen by
// bin_with_atomics() from the sizes alone:
//  * few (workgroup, region) pairs (small scenes, a rank's strip): publish_region_hist above -- no launch of its own, and
//    K3 forms the region starts itself.  At C2 the two scan launches it replaces cost 10 of the mapper's 80 us;
//  * many (C3: 977 workgroups x 256 regions = 250 k pairs): returning atomics on 256 counters run at ~30 G/s and cost the
//    binning pass 8 us, more than the scan launches (K2a + K2b, 5 + 5 us at any size) they save.
// K2a: one workgroup per region: exclusive scan of part[region][*] in place, total -> region_count.
__global__ __launch_bounds__(1024) void region_part_scan_kernel(int num_wg, int* part, int* region_count) {
  __shared__ int s_wave[16];
  const int total = block_scan_row_in_place(part + int64_t(blockIdx.x) * num_wg, num_wg, s_wave);
  if (threadIdx.x == 0) region_count[blockIdx.x] = total;
}

// Exclusive scan of the region populations (thread t = region t; num_regions <= MAX_REGIONS = 1024 threads) -> start of
// each region in the ordered list, returned to every thread for its region.  publish (uniform over the workgroup): the
// starts, and those of the per-region chunk counts (a chunk = up to CHUNK Gaussians of ONE region = one workgroup of
// the counting / bucketing passes), also go to global memory, each with its total appended.
__device__ __forceinline__ int scan_region_starts(int num_regions, const int* region_count, int* s_wave, bool publish,
                                                  int* region_start, int* chunk_start) {
  const int r = threadIdx.x;
  const int c = r < num_regions ? region_count[r] : 0;
  int total_c;
  const int start = block_exclusive_scan(c, s_wave, total_c);
  if (publish) {
    int total_ch;
    const int chunk = block_exclusive_scan((c + CHUNK - 1) / CHUNK, s_wave, total_ch);
    if (r < num_regions) {
      region_start[r] = start;
      chunk_start[r] = chunk;
    }
    if (r == 0) {
      region_start[num_regions] = total_c;
      chunk_start[num_regions] = total_ch;
    }
  }
  return start;
}

// K2b: the region and chunk starts as a launch of their own, behind K2a.
__global__ __launch_bounds__(1024) void region_scan_kernel(int num_regions, const int* region_count, int* region_start,
                                                           int* chunk_start) {
  __shared__ int s_wave[16];
  scan_region_starts(num_regions, region_count, s_wave, true, region_start, chunk_start);
}

// K3: write the Gaussian indices grouped by region: position = region start + this workgroup's offset inside the region
// (K1's atomic) + rank inside the workgroup (LDS atomic).  The region starts are the exclusive scan of the <= 1 024 region
// counters, which every workgroup forms for itself in LDS (4 KB out of L2) instead of reading it from a scan launch;
// workgroup 0 also leaves it -- and the per-region chunk starts (a chunk = up to CHUNK Gaussians of ONE region = one
// workgroup of the counting / bucketing passes) -- in global memory for those passes, and the whole grid clears the tile
// histogram the counting pass adds into.
__global__ __launch_bounds__(BIN) void region_scatter_kernel(RegionGrid rg, int num_wg, const int* region_of,
                                                             const int* part, const int* region_count,
                                                             int* region_start, int* chunk_start,
                                                             const int* block_start, int* order, int* tile_hist,
                                                             int num_tiles, int scanned) {
  __shared__ int s_cnt[MAX_REGIONS];
  __shared__ int s_start[MAX_REGIONS];
  __shared__ int s_wave[16];
  for (int i = blockIdx.x * BIN + threadIdx.x; i < num_tiles; i += gridDim.x * BIN) tile_hist[i] = 0;
  const int t = threadIdx.x;  // num_regions <= MAX_REGIONS = BIN
  s_cnt[t] = 0;
  if (scanned) {  // K2a / K2b have run: the starts are in global memory
    s_start[t] = t < rg.num_regions ? region_start[t] : 0;
  } else {  // workgroup 0 leaves them there for the counting and bucketing passes
    s_start[t] = scan_region_starts(rg.num_regions, region_count, s_wave, blockIdx.x == 0, region_start, chunk_start);
  }
  __syncthreads();
  const int first = block_start[blockIdx.x];
  const int i = first + t;
  if (i < block_start[blockIdx.x + 1]) {
    const int r = region_of[i];
    if (r >= 0) {
      const int local = atomicAdd(&s_cnt[r], 1);
      order[s_start[r] + part[int64_t(r) * num_wg + blockIdx.x] + local] = i;
    }
  }
}

// The projection's stable compaction (project.hip: compact_kernel, whose outputs these are, bit for bit) with K1 folded
// in: a workgroup of BIN = 1024 staged rows writes its visible ones -- one contiguous range of compact rows -- and, while
// it still holds them in registers, runs K1's query on them.  Frame calls only (gs_project_fwd_ex with a GsMapBinPlan).
__global__ __launch_bounds__(BIN) void compact_bin_kernel(GsCompactArgs c, MapArgs a, RegionGrid rg, int num_wg,
                                                          int* region_of, int* part, int* touched_blocks,
                                                          int* block_start, int* region_count) {
  __shared__ int s_hist[MAX_REGIONS];
  for (int r = threadIdx.x; r < rg.num_regions; r += BIN) s_hist[r] = 0;
  const int64_t i = int64_t(blockIdx.x) * BIN + threadIdx.x;
  const float4* st_rows = static_cast<const float4*>(c.st_rows);
  float4 r0 = make_float4(0, 0, 0, 0), r1 = r0;
  bool vis = false;
  if (i < c.n) {
    r0 = st_rows[2 * i];
    r1 = st_rows[2 * i + 1];
    vis = r1.w != 0.0f;
  }
  // the projection pass counted per 256 Gaussians (BIN / 256 of its workgroups in front of each of ours, all of them
  // inside num_blocks); the barrier in here also covers the zeroed histogram
  const int first_small = int(blockIdx.x) * (BIN / 256);
  const GsCompactSlot k = gs_stable_compact<BIN / 64>(vis, c.block_offsets ? c.block_offsets + first_small : nullptr,
                                                      c.block_counts, first_small);
  const int first = k.first, mine_total = k.total;
  if (i < c.n) {
    if (vis) gs_write_compact_row(c, k.slot, i, r0, r1);
    c.slot_of[i] = vis ? k.slot : -1;
  }
  // K1 on the row in registers
  const float g[7] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z};
  bin_row(vis, g, a, rg, region_of + k.slot, s_hist, first, mine_total, num_wg, touched_blocks, block_start);
  if (threadIdx.x == 0 && int(blockIdx.x) == num_wg - 1) *c.num_visible = first + mine_total;
  // the returning atomics of publish_region_hist are issued first and their results stored last: the zero fill of the
  // gradient rows -- a third of this pass's traffic -- runs underneath their latency (num_regions <= BIN: one region
  // per thread)
  const int my_hist = int(threadIdx.x) < rg.num_regions ? s_hist[threadIdx.x] : 0;
  int my_offset = my_hist;
  if (region_count != nullptr && my_hist > 0) my_offset = atomicAdd(region_count + threadIdx.x, my_hist);
  if (c.zero_rows) {  // the frame's gradient rows, cleared by the pass that streams the V rows anyway (project.hip)
    float4* dst = static_cast<float4*>(c.zero_rows) + int64_t(first) * c.zero_row_v4;
    for (int e = threadIdx.x; e < mine_total * c.zero_row_v4; e += BIN) dst[e] = make_float4(0, 0, 0, 0);
  }
  if (int(threadIdx.x) < rg.num_regions && (region_count == nullptr || my_hist > 0))
    part[int64_t(threadIdx.x) * num_wg + blockIdx.x] = my_offset;
}

// which chunk of which region does this workgroup process?
__device__ __forceinline__ bool locate_chunk(int block, const RegionGrid& rg, const int* region_start,
                                             const int* chunk_start, int& region, int& first, int& count) {
  __shared__ int s_loc[3];
  if (threadIdx.x == 0) {
    int r = -1;
    if (block < chunk_start[rg.num_regions]) {
      int lo = 0, hi = rg.num_regions;  // last r with chunk_start[r] <= block
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_start[mid] <= block) lo = mid; else hi = mid;
      }
      r = lo;
      const int c = block - chunk_start[r];
      s_loc[1] = region_start[r] + c * CHUNK;
      s_loc[2] = min(CHUNK, region_start[r + 1] - s_loc[1]);
    }
    s_loc[0] = r;
  }
  __syncthreads();
  region = s_loc[0];
  first = s_loc[1];
  count = s_loc[2];
  return region >= 0;
}

// K4: per-tile histogram through the LDS window.
__global__ __launch_bounds__(CHUNK) void count_binned_kernel(MapArgs a, RegionGrid rg, const int* order,
                                                           const int* region_start, const int* chunk_start,
                                                           int* tile_hist, QueryCache* qcache) {
  extern __shared__ int s_win[];  // win * win
  const int WIN_TILES = rg.win * rg.win;
  int region, first, count;
  if (!locate_chunk(blockIdx.x, rg, region_start, chunk_start, region, first, count)) return;
  for (int e = threadIdx.x; e < WIN_TILES; e += CHUNK) s_win[e] = 0;
  __syncthreads();
  const Window w(rg, region);
  auto add_tile = [&](int gx, int gy) {  // an owned tile
    int e;
    if (w.slot(gx, gy, e)) atomicAdd(&s_win[e], 1);
    else atomicAdd(tile_hist + local_tile(a, gx, gy), 1);
  };
  int i = 0;
  bool wide = false;
  if (int(threadIdx.x) < count) {
    i = order[first + threadIdx.x];
    const GridQuery q = grid_query(a.points + 7 * int64_t(i), a.Wp, a.Hp, a.tile_size, a.thr);
    wide = q.span_x * q.span_y > WIDE_SPAN;
    QueryCache qc;
    qc.accept = 0ull;
    qc.x = unsigned(q.min_tx) | (wide ? 0u : unsigned(q.span_x) << 20);
    qc.y = unsigned(q.min_ty) | (wide ? QC_WIDE : unsigned(q.span_y) << 20);
    if (!wide) {
      int bit = 0;
      for (int ty = 0; ty < q.span_y; ++ty)
        for (int tx = 0; tx < q.span_x; ++tx, ++bit)
          if (gs_shard_owns(a.sh, ty + q.min_ty) && test_tile(q, tx, ty, a.tile_size)) {
            qc.accept |= 1ull << bit;
            add_tile(tx + q.min_tx, ty + q.min_ty);
          }
    }
    // by position in the region order: the bucketing pass reads it back with consecutive 16-byte loads
    *reinterpret_cast<uint4*>(qcache + first + threadIdx.x) = *reinterpret_cast<const uint4*>(&qc);
  }
  for_each_wide_tile(a, i, __ballot(wide), [&](int) { return add_tile; });
  __syncthreads();
  for (int e = threadIdx.x; e < WIN_TILES; e += CHUNK) {
    const int c = s_win[e];
    if (c > 0) {
      int gx, gy;
      w.tile_of(e, gx, gy);
      atomicAdd(tile_hist + local_tile(a, gx, gy), c);
    }
  }
}

// K6: bucket the (depth key, index) pairs.  Pass A counts into the LDS window, pass B reserves one
// contiguous range per window tile with a single returning global atomic, pass C places the pairs
// with LDS atomics.  The accepted-tile set of a lane is kept as a 64-bit mask between the passes
// (so the OBB tests run once); splats whose candidate span exceeds 64 tiles are walked by the whole wave.
__global__ __launch_bounds__(CHUNK) void emit_binned_kernel(MapArgs a, RegionGrid rg, const int* order,
                                                          const int* region_start, const int* chunk_start,
                                                          int* cursors, uint64_t* pairs, const QueryCache* qcache) {
  extern __shared__ int s_dyn[];  // 2 * win * win
  const int WIN_TILES = rg.win * rg.win;
  int* s_cnt = s_dyn;
  int* s_base = s_dyn + WIN_TILES;
  int region, first, count;
  if (!locate_chunk(blockIdx.x, rg, region_start, chunk_start, region, first, count)) return;
  for (int e = threadIdx.x; e < WIN_TILES; e += CHUNK) s_cnt[e] = 0;
  __syncthreads();
  const Window w(rg, region);
  const bool active = int(threadIdx.x) < count;
  unsigned long long accept = 0ull;
  int min_tx = 0, min_ty = 0, span_x = 1;
  bool wide = false;  // candidate span above WIDE_SPAN tiles: walked by the whole wave in both passes
  int i = 0;
  auto count_tile = [&](int gx, int gy) {
    int e;
    if (w.slot(gx, gy, e)) atomicAdd(&s_cnt[e], 1);
  };
  if (active) {
    i = order[first + threadIdx.x];
    const uint4 raw = *reinterpret_cast<const uint4*>(qcache + first + threadIdx.x);
    const QueryCache qc = *reinterpret_cast<const QueryCache*>(&raw);
    wide = (qc.y & QC_WIDE) != 0u;
    if (!wide) {
      accept = qc.accept;
      min_tx = qc_min_tx(qc); min_ty = qc_min_ty(qc); span_x = qc_span_x(qc);
      for_each_accepted(accept, span_x, [&](int tx, int ty) { count_tile(tx + min_tx, ty + min_ty); });
    }
  }
  const uint64_t wide_lanes = __ballot(wide);
  for_each_wide_tile(a, i, wide_lanes, [&](int) { return count_tile; });
  __syncthreads();
  for (int e = threadIdx.x; e < WIN_TILES; e += CHUNK) {
    const int c = s_cnt[e];
    if (c > 0) {
      int gx, gy;
      w.tile_of(e, gx, gy);
      // a tile dropped by the capacity clamp has a hugely negative cursor: the returned value says so
      // (no separate load in front of the atomic: the reservations of a workgroup must pipeline)
      const int base = atomicAdd(cursors + local_tile(a, gx, gy), c);
      s_base[e] = base < 0 ? -1 : base;
    }
    s_cnt[e] = 0;
  }
  __syncthreads();
  auto place = [&](int gx, int gy, uint64_t pair) {
    int e;
    int slot;
    if (w.slot(gx, gy, e)) {
      if (s_base[e] < 0) return;
      slot = s_base[e] + atomicAdd(&s_cnt[e], 1);
    } else {
      slot = atomicAdd(cursors + local_tile(a, gx, gy), 1);
      if (slot < 0) return;
    }
    pairs[slot] = pair;
  };
  auto pair_of = [&](int gi) {
    return (uint64_t(depth_key(a.depth[gi], a.depth16 != 0)) << 32) | uint64_t(uint32_t(gi));
  };
  if (active && !wide) {
    const uint64_t pair = pair_of(i);
    for_each_accepted(accept, span_x, [&](int tx, int ty) { place(tx + min_tx, ty + min_ty, pair); });
  }
  for_each_wide_tile(a, i, wide_lanes, [&](int gi) {
    const uint64_t pair = pair_of(gi);
    return [&place, pair](int gx, int gy) { place(gx, gy, pair); };
  });
}

struct MapScratch {
  int* hist; int* cursors; int* region_of; int* order; int* region_count; int* region_start; int* part;
  int* chunk_start;
  QueryCache* qcache;
  int* touched_blocks;  // per 1024-row workgroup of the binning pass: rows that entered the ordering
  int* block_start;     // rows of workgroup b of the binning pass: [block_start[b], block_start[b + 1])
  char* end;            // one past the layout: gs_map_scratch_bytes
};
// part[region][workgroup]; the region count is bounded by the tile count and by MAX_REGIONS
int64_t part_entries(int64_t v, int64_t num_tiles) {
  const int64_t regions = num_tiles < MAX_REGIONS ? (num_tiles < 1 ? 1 : num_tiles) : MAX_REGIONS;
  return regions * gs_div_up(v > 0 ? v : 1, BIN);
}
MapScratch carve(void* scratch, int64_t v, int64_t num_tiles) {
  char* p = static_cast<char*>(scratch);
  MapScratch m;
  auto take = [&](int64_t bytes) { int* r = reinterpret_cast<int*>(p); p += gs_align_up(bytes, 256); return r; };
  m.hist = take(num_tiles * 4);
  m.cursors = take(num_tiles * 4);
  m.region_of = take(v * 4);
  m.order = take(v * 4);
  m.region_count = take((MAX_REGIONS + 1) * 4);
  m.region_start = take((MAX_REGIONS + 1) * 4);
  m.chunk_start = take((MAX_REGIONS + 1) * 4);
  m.part = take(part_entries(v, num_tiles) * 4);
  m.qcache = reinterpret_cast<QueryCache*>(take(v * int64_t(sizeof(QueryCache))));
  m.touched_blocks = take((gs_div_up(v > 0 ? v : 1, BIN) + 1) * 4);
  m.block_start = take((gs_div_up(v > 0 ? v : 1, BIN) + 1) * 4);
  m.end = p;
  return m;
}
RegionGrid make_grid(const MapArgs& a) {
  RegionGrid rg;
  rg.tiles_x = a.tiles_wide;
  rg.row0 = a.sh.period == 1 ? a.sh.begin : 0;
  rg.tiles_y = a.sh.period == 1 ? a.sh.end - a.sh.begin : a.Hp / a.tile_size;
  rg.rg = RG_MIN;
  while (gs_div_up(rg.tiles_x, rg.rg) * gs_div_up(rg.tiles_y, rg.rg) > MAX_REGIONS) rg.rg *= 2;
  rg.win = rg.rg + 2 * RB;
  rg.regions_x = int(gs_div_up(rg.tiles_x, rg.rg));
  rg.num_regions = rg.regions_x * int(gs_div_up(rg.tiles_y, rg.rg));
  return rg;
}

// (workgroup, region) pairs up to which the binning pass reserves its places with atomics (see K1 / K2)
bool bin_with_atomics(int64_t num_wg, const RegionGrid& rg) { return num_wg * rg.num_regions <= (int64_t(1) << 16); }

// ascending list of the rows with region_of >= 0: a stable compaction on the per-workgroup counts the binning pass
// left (every workgroup adds up the counts in front of it, as the projection's compaction does)
__global__ __launch_bounds__(1024) void touched_write_kernel(const int* block_start, const int* region_of,
                                                             const int* block_counts, int* touched, int* count_out) {
  const int i = block_start[blockIdx.x] + int(threadIdx.x);  // the binning pass's own rows (ascending over workgroups)
  const bool flag = i < block_start[blockIdx.x + 1] && region_of[i] >= 0;
  const GsCompactSlot k = gs_stable_compact<16>(flag, nullptr, block_counts, int(blockIdx.x));
  if (flag) touched[k.slot] = i;
  if (count_out && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *count_out = k.first + k.total;
}

// owner r's share of the ascending list: [first row whose Gaussian index >= r chunk, ... (r + 1) chunk)
__global__ void owner_cuts_kernel(const int* block_counts, int num_blocks, const int* touched, const int64_t* indexes,
                                  int64_t chunk, int world, int64_t* owner_counts, const int* v_dev, int64_t v,
                                  int owner, int* owned_rows) {
  __shared__ int64_t s_cut[65];
  __shared__ int s_part[128];
  const int t = threadIdx.x;
  int part = 0;
  for (int j = t; j < num_blocks; j += 128) part += block_counts[j];
  s_part[t] = part;
  __syncthreads();
  int m = 0;
  for (int j = 0; j < 128; ++j) m += s_part[j];
  if (t <= world) {
    const int64_t bound = int64_t(t) * chunk;
    int lo = 0, hi = m;  // first e with indexes[touched[e]] >= bound
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (indexes[touched[mid]] < bound) lo = mid + 1; else hi = mid;
    }
    s_cut[t] = t == world ? m : lo;
  }
  __syncthreads();
  if (t < world) owner_counts[t] = s_cut[t + 1] - s_cut[t];
  // the rows (of the whole visible list, not only the touched ones) whose Gaussians `owner` owns: [first row with
  // index >= owner chunk, first row with index >= (owner + 1) chunk)
  if (owned_rows && t >= 126) {
    const int64_t bound = int64_t(owner + (t - 126)) * chunk;
    int64_t lo = 0, hi = v_dev ? (int64_t(*v_dev) < v ? int64_t(*v_dev) : v) : v;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (indexes[mid] < bound) lo = mid + 1; else hi = mid;
    }
    owned_rows[t - 126] = int(lo);
  }
}
}  // namespace

extern "C" int64_t gs_map_scratch_bytes(int64_t v, int64_t num_tiles) {
  return carve(nullptr, v, num_tiles).end - static_cast<char*>(nullptr);
}

extern "C" int64_t gs_map_touched_offset(int64_t v, int64_t num_tiles) {
  const MapScratch m = carve(nullptr, v, num_tiles);
  return reinterpret_cast<char*>(m.order) - static_cast<char*>(nullptr);
}

extern "C" int gs_map_touched_list(int64_t v, const int32_t* v_dev, int64_t num_tiles, const void* scratch,
                                   int64_t scratch_bytes, int32_t* touched_out, int32_t* count_out,
                                   const int64_t* indexes, int64_t n, int32_t world, int64_t* owner_counts,
                                   int32_t owner, int32_t* owned_rows, void* stream) {
  GS_REQUIRE(v >= 0 && v < (int64_t(1) << 31) && num_tiles >= 1, GS_ERR_INVALID_ARGUMENT, "gs_map_touched_list: sizes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (owner_counts) {
    GS_REQUIRE(world >= 1 && world <= 64 && indexes && n >= 0, GS_ERR_INVALID_ARGUMENT,
               "gs_map_touched_list: %d owners (1 .. 64) need the index list", world);
    if (int rc = gs_memset_async(owner_counts, size_t(world) * 8, s, "gs_map_touched_list: hipMemsetAsync failed"))
      return rc;
  }
  if (count_out && v == 0)
    if (int rc = gs_memset_async(count_out, 4, s, "gs_map_touched_list: hipMemsetAsync failed")) return rc;
  if (v == 0) return GS_OK;
  const int nb = int(gs_div_up(v, 1024));
  GS_REQUIRE(scratch && scratch_bytes >= gs_map_scratch_bytes(v, num_tiles), GS_ERR_SCRATCH_TOO_SMALL,
             "gs_map_touched_list: scratch is not the one gs_map_prepare filled");
  GS_REQUIRE(touched_out, GS_ERR_INVALID_ARGUMENT, "gs_map_touched_list: touched_out is NULL");
  const MapScratch m = carve(const_cast<void*>(scratch), v, num_tiles);
  const int* block_counts = m.touched_blocks;  // BIN = 1024 rows per workgroup of the binning pass
  hipLaunchKernelGGL(touched_write_kernel, dim3(nb), dim3(1024), 0, s, m.block_start, m.region_of, block_counts,
                     touched_out, count_out);
  if (owner_counts) {
    GS_REQUIRE(!owned_rows || (owner >= 0 && owner < world), GS_ERR_INVALID_ARGUMENT,
               "gs_map_touched_list: owned_rows needs the owner's rank");
    hipLaunchKernelGGL(owner_cuts_kernel, dim3(1), dim3(128), 0, s, block_counts, nb, touched_out, indexes,
                       gs_div_up(n > 0 ? n : 1, world), world, owner_counts, v_dev, v, owner, owned_rows);
  }
  GS_CHECK_LAUNCH("gs_map_touched_list");
  return GS_OK;
}

// the region counters of the plan's mapper scratch: whoever runs in front of the binning pass clears them (the frame
// calls: the projection's first pass; standalone: a memset)
int gs_map_bin_counters(const GsMapBinPlan* plan, int64_t n, int32_t** words, int32_t* count) {
  MapArgs a;
  if (int rc = fill_args(a, n, nullptr, nullptr, plan->width, plan->height, plan->cfg, 0, plan->shard)) return rc;
  GS_REQUIRE(a.sh.local_rows > 0 && plan->scratch, GS_ERR_INVALID_ARGUMENT, "gs_map_bin_counters: nothing to bin");
  const MapScratch m = carve(plan->scratch, n, int64_t(a.tiles_wide) * a.sh.local_rows);
  const bool atomics = bin_with_atomics(gs_div_up(n > 0 ? n : 1, BIN), make_grid(a));
  *words = atomics ? m.region_count : nullptr;  // the scan launches write every counter themselves
  *count = atomics ? MAX_REGIONS + 1 : 0;
  return GS_OK;
}

int gs_map_compact_bin(const GsMapBinPlan* plan, const GsCompactArgs* c, void* stream) {
  MapArgs a;
  if (int rc = fill_args(a, c->n, c->points, nullptr, plan->width, plan->height, plan->cfg, 0, plan->shard)) return rc;
  GS_REQUIRE(a.sh.local_rows > 0 && c->n > 0, GS_ERR_INVALID_ARGUMENT, "gs_map_compact_bin: nothing to bin");
  const int num_tiles = a.tiles_wide * a.sh.local_rows;
  GS_REQUIRE(plan->scratch && plan->scratch_bytes >= gs_map_scratch_bytes(c->n, num_tiles), GS_ERR_SCRATCH_TOO_SMALL,
             "gs_map_compact_bin: mapper scratch %lld < %lld bytes", (long long)plan->scratch_bytes,
             (long long)gs_map_scratch_bytes(c->n, num_tiles));
  const RegionGrid rg = make_grid(a);
  GS_REQUIRE(rg.num_regions <= MAX_REGIONS, GS_ERR_UNSUPPORTED, "gs_map_compact_bin: %d regions", rg.num_regions);
  const MapScratch m = carve(plan->scratch, c->n, num_tiles);
  const unsigned vb = unsigned(gs_div_up(c->n, BIN));
  hipLaunchKernelGGL(compact_bin_kernel, dim3(vb), dim3(BIN), 0, static_cast<hipStream_t>(stream), *c, a, rg, int(vb),
                     m.region_of, m.part, m.touched_blocks, m.block_start,
                     bin_with_atomics(vb, rg) ? m.region_count : nullptr);
  GS_CHECK_LAUNCH("gs_map_compact_bin");
  return GS_OK;
}

extern "C" int gs_map_prepare(int64_t v, const int32_t* v_dev, const float* points, int32_t width, int32_t height,
                              const GsRasterConfig* cfg, int64_t k_capacity, int32_t* tile_ranges,
                              int32_t* counts_out, int32_t* counts_host, int32_t* tile_order,
                              const GsRowShard* shard, void* scratch, int64_t scratch_bytes, void* stream) {
  return gs_map_prepare_ex(v, v_dev, points, width, height, cfg, k_capacity, tile_ranges, counts_out, counts_host,
                           tile_order, shard, scratch, scratch_bytes, 0, stream);
}

// binned != 0: gs_map_compact_bin has filled region_of / part / touched_blocks / block_start of `scratch` already
int gs_map_prepare_ex(int64_t v, const int32_t* v_dev, const float* points, int32_t width, int32_t height,
                      const GsRasterConfig* cfg, int64_t k_capacity, int32_t* tile_ranges, int32_t* counts_out,
                      int32_t* counts_host, int32_t* tile_order, const GsRowShard* shard, void* scratch,
                      int64_t scratch_bytes, int binned, void* stream) {
  MapArgs a;
  if (int rc = fill_args(a, v, points, nullptr, width, height, cfg, 0, shard)) return rc;
  a.v_dev = v_dev;
  GS_REQUIRE(a.sh.local_rows > 0, GS_ERR_INVALID_ARGUMENT, "gs_map_prepare: the shard owns no tile row");
  const int num_tiles = a.tiles_wide * a.sh.local_rows;
  GS_REQUIRE(tile_ranges && counts_out && scratch, GS_ERR_INVALID_ARGUMENT, "gs_map_prepare: NULL buffer");
  GS_REQUIRE(scratch_bytes >= gs_map_scratch_bytes(v, num_tiles), GS_ERR_SCRATCH_TOO_SMALL,
             "gs_map_prepare: scratch %lld < %lld bytes", (long long)scratch_bytes,
             (long long)gs_map_scratch_bytes(v, num_tiles));
  GS_REQUIRE(num_tiles <= (1 << 20), GS_ERR_UNSUPPORTED, "gs_map_prepare: %d tiles (limit 2^20)", num_tiles);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const MapScratch m = carve(scratch, v, num_tiles);
  int* hist = m.hist;
  int* cursors = m.cursors;
  const RegionGrid rg = make_grid(a);
  GS_REQUIRE(rg.num_regions <= MAX_REGIONS && rg.win * rg.win * 8 <= 65536, GS_ERR_UNSUPPORTED,
             "gs_map_prepare: tile grid %dx%d needs %d regions of edge %d", rg.tiles_x, rg.tiles_y, rg.num_regions,
             rg.rg);
  if (v == 0)
    if (int rc = gs_memset_async(hist, size_t(num_tiles) * 4, s, "gs_map_prepare: hipMemsetAsync failed")) return rc;
  if (v > 0) {
    GS_REQUIRE(points, GS_ERR_INVALID_ARGUMENT, "gs_map_prepare: points is NULL");
    const unsigned vb = unsigned(gs_div_up(v, BIN));
    const bool atomics = bin_with_atomics(vb, rg);
    if (!binned) {
      if (atomics)
        if (int rc = gs_memset_async(m.region_count, size_t(MAX_REGIONS + 1) * 4, s,
                                     "gs_map_prepare: hipMemsetAsync failed"))
          return rc;
      hipLaunchKernelGGL(region_count_kernel, dim3(vb), dim3(BIN), 0, s, a, rg, int(vb), m.region_of, m.part,
                         m.touched_blocks, m.block_start, atomics ? m.region_count : nullptr);
    }
    if (!atomics) {
      hipLaunchKernelGGL(region_part_scan_kernel, dim3(rg.num_regions), dim3(1024), 0, s, int(vb), m.part,
                         m.region_count);
      hipLaunchKernelGGL(region_scan_kernel, dim3(1), dim3(1024), 0, s, rg.num_regions, m.region_count,
                         m.region_start, m.chunk_start);
    }
    hipLaunchKernelGGL(region_scatter_kernel, dim3(vb), dim3(BIN), 0, s, rg, int(vb), m.region_of, m.part,
                       m.region_count, m.region_start, m.chunk_start, m.block_start, m.order, hist, num_tiles,
                       atomics ? 0 : 1);
    // one workgroup per chunk of <= CHUNK Gaussians of one region; surplus workgroups exit at once
    hipLaunchKernelGGL(count_binned_kernel, dim3(unsigned(gs_div_up(v, CHUNK)) + unsigned(rg.num_regions)), dim3(CHUNK),
                       size_t(rg.win) * rg.win * 4, s, a, rg, m.order,
                       m.region_start, m.chunk_start, hist, m.qcache);
    GS_CHECK_LAUNCH("gs_map_prepare/count");
  }
  hipLaunchKernelGGL(map_scan_kernel, dim3(tile_order ? 2 : 1), dim3(1024), 0, s, num_tiles, hist,
                     reinterpret_cast<int2*>(tile_ranges), cursors, counts_out, k_capacity, tile_order, v_dev,
                     counts_host, v > 0 ? m.region_start + rg.num_regions : nullptr);
  GS_CHECK_LAUNCH("gs_map_prepare/scan");
  return GS_OK;
}

extern "C" int gs_map_finish(int64_t v, const int32_t* v_dev, int64_t k, int32_t max_tile_count, const float* points,
                             const float* depth, int32_t width, int32_t height, const GsRasterConfig* cfg,
                             int32_t use_depth16, const int32_t* tile_ranges, int32_t* overlap_to_point,
                             uint64_t* sorted_keys, void* pair_scratch, const GsRowShard* shard, void* scratch,
                             int64_t scratch_bytes, void* stream) {
  MapArgs a;
  if (int rc = fill_args(a, v, points, depth, width, height, cfg, use_depth16, shard)) return rc;
  a.v_dev = v_dev;
  if (k == 0 || v == 0) return GS_OK;
  const int num_tiles = a.tiles_wide * a.sh.local_rows;
  GS_REQUIRE(points && depth && tile_ranges && overlap_to_point && pair_scratch && scratch, GS_ERR_INVALID_ARGUMENT,
             "gs_map_finish: NULL buffer");
  GS_REQUIRE(scratch_bytes >= gs_map_scratch_bytes(v, num_tiles), GS_ERR_SCRATCH_TOO_SMALL,
             "gs_map_finish: scratch too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const MapScratch m = carve(scratch, v, num_tiles);
  int* cursors = m.cursors;
  const RegionGrid rg = make_grid(a);
  uint64_t* pairs = static_cast<uint64_t*>(pair_scratch);
  // the region ordering left in scratch by gs_map_prepare is reused here
  hipLaunchKernelGGL(emit_binned_kernel, dim3(unsigned(gs_div_up(v, CHUNK)) + unsigned(rg.num_regions)), dim3(CHUNK),
                     size_t(rg.win) * rg.win * 8, s,
                     a, rg, m.order, m.region_start, m.chunk_start, cursors, pairs, m.qcache);
  GS_CHECK_LAUNCH("gs_map_finish/emit");
  return gs_map_sort_tiles(num_tiles, tile_ranges, pairs, overlap_to_point, sorted_keys, use_depth16, max_tile_count, s);
}
