// bilagrid.hip -- slicing a bilateral grid of 3x4 colour transforms, forward and backward (gfx950), float and double.
//
// Per pixel (column x, row y) of a channel-last image, with a grid (12, L, Hg, Wg) whose channel 4 r + c is element
// (r, c) of an affine matrix:
//   gx = (x + 0.5) * (Wg - 1) / W,  gy = (y + 0.5) * (Hg - 1) / H,  gz = clamp(luma, 0, 1) * (L - 1),
//   A = trilinear interpolation at (gz, gy, gx), cell = min(floor(coord), size - 2) (0 when the size is 1),
//   out = A[:, :3] rgb + A[:, 3].
// Interpolation is a + (b - a) * f along x, then y, then z: where the eight corners agree the result is the corner,
// so an identity grid returns the image bit for bit.
//
// One wave per workgroup, one square pixel tile per workgroup.  The host picks the tile edge (32, 16, 8, 4, 2 or 1
// pixels) so that the block of grid nodes the tile's pixels touch -- all L levels, all 12 channels -- fits in LDS twice
// (the backward keeps the nodes and their gradient sums); host and device find a tile's block with the same two
// rounded operations per axis (bg_cell), so the host's bound is the device's extent.  The wave walks the tile 64
// pixels at a time.
//
// Backward, grid gradient: a pixel adds weight(corner) * d_out[r] * (rgb[c] | 1) to 8 corners x 12 channels.  Lanes
// of a wave mostly share a cell, so the wave takes the cells present among its 64 pixels one after the other (in the
// order of the first lane holding each), reduces the 96 products of the lanes in that cell with six 16-value
// transposed butterflies (gs_wave_reduce16_transposed: lane l ends with the total of value l / 4) and sixteen owner
// lanes add the totals to the tile's sums in LDS.  One wave, one program order: no atomics, and the sums repeat bit
// for bit.  The tile's sums go to scratch; a second launch adds, per grid element, the sums of the tiles that reach
// it, in an order the shapes fix, in double.
#include <cmath>

#include "gs_common.h"

namespace {

constexpr int BG_CH = 12;
constexpr int BG_LDS_BYTES = 64 * 1024;
constexpr int BG_TILES[] = {32, 16, 8, 4, 2, 1};
constexpr int BG_NUM_TILES = 6;
constexpr int64_t BG_MIN_GROUPS = 1024;  // a tile edge above 8 only while it leaves one wave for every SIMD of the chip

template <typename T>
struct BgImage {
  const T* p;
  int64_t sb, sr, sp;
};

template <typename T>
struct BgArgs {
  int batch, height, width;
  int L, Hg, Wg;
  int tile, tile_shift, tiles_x, tiles_y;
  int block_elems;  // elements of one workgroup's slot in `partials`: the largest block of any tile
  T sx, sy, sz;     // (Wg - 1) / W, (Hg - 1) / H, L - 1
  BgImage<T> x, guide;  // guide.p == NULL: the image's luma
  const T* grid;
  int64_t grid_sb;
  T* out;             // forward
  const T* grad_out;  // backward: (B, H, W, 3) contiguous
  T* d_image;         // (B, H, W, 3) contiguous, or NULL
  T* d_guide;         // (B, H, W) contiguous, or NULL
  T* partials;        // NULL: no grid gradient
};

// cell and fraction of pixel (or row) i along an axis of `size` nodes.  An add and a multiply, each rounded once, on
// host and device alike; monotone in i.
template <typename T>
GS_HD int bg_cell(int i, T scale, int size, T* frac) {
  const T g = (T(i) + T(0.5)) * scale;
  int c = int(g);
  c = c < size - 2 ? c : size - 2;
  c = c < 0 ? 0 : c;
  *frac = g - T(c);
  return c;
}

// the nodes [b0, b0 + nb) that the pixels [t0, min(t0 + tile, extent)) touch along one axis
template <typename T>
GS_HD void bg_block(int t0, int tile, int extent, T scale, int size, int* b0, int* nb) {
  T f;
  const int last = (t0 + tile < extent ? t0 + tile : extent) - 1;
  const int c0 = bg_cell(t0, scale, size, &f), c1 = bg_cell(last, scale, size, &f);
  const int hi = c1 + 1 < size ? c1 + 1 : size - 1;
  *b0 = c0;
  *nb = hi - c0 + 1;
}

template <typename T>
struct BgTile {
  int b, x0, y0, bx0, nbx, by0, nby;
};

template <typename T>
__device__ __forceinline__ BgTile<T> bg_tile(const BgArgs<T>& a, int t) {
  BgTile<T> k;
  const int tx = t % a.tiles_x;
  t /= a.tiles_x;
  const int ty = t % a.tiles_y;
  k.b = t / a.tiles_y;
  k.x0 = tx * a.tile;
  k.y0 = ty * a.tile;
  bg_block(k.x0, a.tile, a.width, a.sx, a.Wg, &k.bx0, &k.nbx);
  bg_block(k.y0, a.tile, a.height, a.sy, a.Hg, &k.by0, &k.nby);
  return k;
}

// the tile's block of the grid -> LDS, node-major: s[((z * nby + y) * nbx + x) * 12 + channel]
template <typename T>
__device__ __forceinline__ void bg_stage(const BgArgs<T>& a, const BgTile<T>& k, T* s, int lane) {
  const int n = BG_CH * a.L * k.nby * k.nbx;
  const T* g = a.grid + int64_t(k.b) * a.grid_sb;
  for (int e = lane; e < n; e += GS_WAVE) {
    const int xx = e % k.nbx;
    int r = e / k.nbx;
    const int yy = r % k.nby;
    r /= k.nby;
    const int z = r % a.L, c = r / a.L;
    s[((z * k.nby + yy) * k.nbx + xx) * BG_CH + c] =
        g[((int64_t(c) * a.L + z) * a.Hg + (k.by0 + yy)) * a.Wg + (k.bx0 + xx)];
  }
}

// where a pixel sits in its tile's block
template <typename T>
struct BgPixel {
  int lx, ly, cz;  // cell, x and y relative to the block
  int hx, hy, hz;  // 1 when the axis has a node above the cell (size > 1)
  T fx, fy, fz;
  bool inside;     // the guide lies strictly inside (0, 1): gz carries a gradient
};

template <typename T>
__device__ __forceinline__ BgPixel<T> bg_locate(const BgArgs<T>& a, const BgTile<T>& k, int px, int py, T luma) {
  BgPixel<T> q;
  const int cx = bg_cell(px, a.sx, a.Wg, &q.fx), cy = bg_cell(py, a.sy, a.Hg, &q.fy);
  q.lx = cx - k.bx0;
  q.ly = cy - k.by0;
  q.hx = cx + 1 < a.Wg;
  q.hy = cy + 1 < a.Hg;
  q.hz = a.L > 1;
  q.inside = luma > T(0) && luma < T(1);
  // fmin / fmax drop a NaN: the cell stays inside the block whatever the pixel holds
  const T gz = fmax(fmin(luma, T(1)), T(0)) * a.sz;
  int cz = int(gz);
  cz = cz < a.L - 2 ? cz : a.L - 2;
  cz = cz < 0 ? 0 : cz;
  q.cz = cz;
  q.fz = gz - T(cz);
  return q;
}

// bilinear interpolation of the 12 channels on level z of the block
template <typename T>
__device__ __forceinline__ void bg_plane(const T* s, const BgTile<T>& k, const BgPixel<T>& q, int z, T (&P)[BG_CH]) {
  const int n00 = ((z * k.nby + q.ly) * k.nbx + q.lx) * BG_CH;
  const int n01 = n00 + q.hx * BG_CH;
  const int n10 = n00 + q.hy * k.nbx * BG_CH;
  const int n11 = n10 + q.hx * BG_CH;
#pragma unroll
  for (int c = 0; c < BG_CH; ++c) {
    const T v00 = s[n00 + c], v01 = s[n01 + c], v10 = s[n10 + c], v11 = s[n11 + c];
    const T top = v00 + (v01 - v00) * q.fx;
    const T bot = v10 + (v11 - v10) * q.fx;
    P[c] = top + (bot - top) * q.fy;
  }
}

template <typename T>
__device__ __forceinline__ T bg_luma(T r, T g, T b) {
  return T(0.299) * r + T(0.587) * g + T(0.114) * b;
}

template <typename T>
__global__ __launch_bounds__(GS_WAVE) void bilagrid_fwd_kernel(BgArgs<T> a) {
  extern __shared__ __align__(16) unsigned char bg_smem[];
  T* s_grid = reinterpret_cast<T*>(bg_smem);
  const int lane = threadIdx.x;
  const BgTile<T> k = bg_tile(a, int(blockIdx.x));
  bg_stage(a, k, s_grid, lane);
  __syncthreads();
  const int pixels = a.tile * a.tile;
  for (int p = lane; p < pixels; p += GS_WAVE) {
    const int px = k.x0 + (p & (a.tile - 1)), py = k.y0 + (p >> a.tile_shift);
    if (px >= a.width || py >= a.height) continue;
    const T* xp = a.x.p + int64_t(k.b) * a.x.sb + int64_t(py) * a.x.sr + int64_t(px) * a.x.sp;
    const T r = xp[0], g = xp[1], b = xp[2];
    const T luma = a.guide.p ? a.guide.p[int64_t(k.b) * a.guide.sb + int64_t(py) * a.guide.sr + int64_t(px) * a.guide.sp]
                             : bg_luma(r, g, b);
    const BgPixel<T> q = bg_locate(a, k, px, py, luma);
    T P0[BG_CH], P1[BG_CH];
    bg_plane(s_grid, k, q, q.cz, P0);
    bg_plane(s_grid, k, q, q.cz + q.hz, P1);
    T* o = a.out + ((int64_t(k.b) * a.height + py) * a.width + px) * 3;
#pragma unroll
    for (int row = 0; row < 3; ++row) {
      T A[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) A[c] = P0[4 * row + c] + (P1[4 * row + c] - P0[4 * row + c]) * q.fz;
      o[row] = A[0] * r + A[1] * g + A[2] * b + A[3];
    }
  }
}

// the totals of 16 values over the wave, lane l holding that of value l / 4
__device__ __forceinline__ float bg_reduce16(float (&v)[16], int lane) { return gs_wave_reduce16_transposed(v, lane); }

__device__ __forceinline__ double bg_reduce16(double (&v)[16], int lane) {  // gradcheck only: sixteen xor butterflies
  double mine = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    double t = v[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
    mine = (lane >> 2) == i ? t : mine;
  }
  return mine;
}

template <typename T>
__global__ __launch_bounds__(GS_WAVE) void bilagrid_bwd_kernel(BgArgs<T> a) {
  const int lane = threadIdx.x;
  const BgTile<T> k = bg_tile(a, int(blockIdx.x));
  const int block = BG_CH * a.L * k.nby * k.nbx;
  extern __shared__ __align__(16) unsigned char bg_smem[];
  T* s_grid = reinterpret_cast<T*>(bg_smem);
  T* s_acc = s_grid + block;
  bg_stage(a, k, s_grid, lane);
  for (int e = lane; e < block; e += GS_WAVE) s_acc[e] = T(0);
  __syncthreads();
  const int pixels = a.tile * a.tile;
  const int passes = (pixels + GS_WAVE - 1) / GS_WAVE;
  for (int pass = 0; pass < passes; ++pass) {
    const int p = pass * GS_WAVE + lane;
    const int px = k.x0 + (p & (a.tile - 1)), py = k.y0 + (p >> a.tile_shift);
    const bool active = p < pixels && px < a.width && py < a.height;
    T v[BG_CH];
    T w[8];
    int key = -1;
    if (active) {
      const T* xp = a.x.p + int64_t(k.b) * a.x.sb + int64_t(py) * a.x.sr + int64_t(px) * a.x.sp;
      const T r = xp[0], g = xp[1], b = xp[2];
      const T luma = a.guide.p
                         ? a.guide.p[int64_t(k.b) * a.guide.sb + int64_t(py) * a.guide.sr + int64_t(px) * a.guide.sp]
                         : bg_luma(r, g, b);
      const BgPixel<T> q = bg_locate(a, k, px, py, luma);
      const int64_t pix = (int64_t(k.b) * a.height + py) * a.width + px;
      const T* go = a.grad_out + pix * 3;
      const T d[3] = {go[0], go[1], go[2]};
      T P0[BG_CH], P1[BG_CH];
      bg_plane(s_grid, k, q, q.cz, P0);
      bg_plane(s_grid, k, q, q.cz + q.hz, P1);
      T dr = T(0), dg = T(0), db = T(0), dz = T(0);
#pragma unroll
      for (int row = 0; row < 3; ++row) {
        v[4 * row] = d[row] * r;
        v[4 * row + 1] = d[row] * g;
        v[4 * row + 2] = d[row] * b;
        v[4 * row + 3] = d[row];
        T A[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) A[c] = P0[4 * row + c] + (P1[4 * row + c] - P0[4 * row + c]) * q.fz;
        dr += d[row] * A[0];
        dg += d[row] * A[1];
        db += d[row] * A[2];
#pragma unroll
        for (int c = 0; c < 4; ++c) dz += v[4 * row + c] * (P1[4 * row + c] - P0[4 * row + c]);
      }
      const T dl = q.inside ? dz * a.sz : T(0);
      if (a.guide.p) {
        if (a.d_guide) a.d_guide[pix] = dl;
      } else {
        dr += T(0.299) * dl;
        dg += T(0.587) * dl;
        db += T(0.114) * dl;
      }
      if (a.d_image) {
        a.d_image[pix * 3] = dr;
        a.d_image[pix * 3 + 1] = dg;
        a.d_image[pix * 3 + 2] = db;
      }
      const T wx[2] = {T(1) - q.fx, q.fx}, wy[2] = {T(1) - q.fy, q.fy}, wz[2] = {T(1) - q.fz, q.fz};
#pragma unroll
      for (int corner = 0; corner < 8; ++corner) w[corner] = wz[corner >> 2] * wy[(corner >> 1) & 1] * wx[corner & 1];
      key = (q.cz * k.nby + q.ly) * k.nbx + q.lx;  // the cell's lowest node in the block
    } else {
#pragma unroll
      for (int c = 0; c < BG_CH; ++c) v[c] = T(0);
#pragma unroll
      for (int corner = 0; corner < 8; ++corner) w[corner] = T(0);
    }
    if (!a.partials) continue;
    // the cells among the wave's pixels, one after the other
    uint64_t todo = __ballot(active);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int cell = __shfl(key, leader);
      const bool in = key == cell;
      T m[BG_CH];
#pragma unroll
      for (int c = 0; c < BG_CH; ++c) m[c] = in ? v[c] : T(0);
#pragma unroll
      for (int group = 0; group < 6; ++group) {
        T vals[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) vals[i] = w[(16 * group + i) / BG_CH] * m[(16 * group + i) % BG_CH];
        const T total = bg_reduce16(vals, lane);
        const int j = 16 * group + (lane >> 2), corner = j / BG_CH, c = j - BG_CH * corner;
        const int ox = corner & 1, oy = (corner >> 1) & 1, oz = corner >> 2;
        // an axis of one node has no upper corner: its weight is exactly zero, and its node is the lower corner's
        const bool exists = (!ox || a.Wg > 1) && (!oy || a.Hg > 1) && (!oz || a.L > 1);
        if ((lane & 3) == 0 && exists) s_acc[(cell + (oz * k.nby + oy) * k.nbx + ox) * BG_CH + c] += total;
      }
      todo &= ~__ballot(in);
      __syncthreads();  // one wave: orders the owner lanes' sums of this cell before those of the next
    }
  }
  if (!a.partials) return;
  __syncthreads();
  T* out = a.partials + int64_t(blockIdx.x) * a.block_elems;
  for (int e = lane; e < block; e += GS_WAVE) out[e] = s_acc[e];
}

// d_grid[b, :, z, y, x]: one workgroup per node adds the sums of the tiles whose block holds node (y, x).  Those tiles
// are a rectangle of tiles (a block's first and last node ascend with the tile); its corners come from integer LDS
// min / max.  Thread (slice s, channel c) adds the rectangle's tiles s, s + 85, ... in double, thread c then the 85
// slices in order: the order of the additions depends on the shapes alone.
constexpr int BG_FIN_SLICES = 85, BG_FIN_THREADS = 1024;

template <typename T>
__global__ __launch_bounds__(BG_FIN_THREADS) void bilagrid_finish_kernel(BgArgs<T> a, T* d_grid) {
  __shared__ int s_range[4];  // first and last tile row, first and last tile column
  __shared__ double s_part[BG_FIN_SLICES][BG_CH];
  const int tid = threadIdx.x;
  int e = int(blockIdx.x);
  const int x = e % a.Wg;
  e /= a.Wg;
  const int y = e % a.Hg;
  e /= a.Hg;
  const int z = e % a.L, b = e / a.L;
  if (tid < 4) s_range[tid] = (tid & 1) ? -1 : 0x7fffffff;
  __syncthreads();
  for (int t = tid; t < a.tiles_y + a.tiles_x; t += BG_FIN_THREADS) {
    const bool row = t < a.tiles_y;
    const int i = row ? t : t - a.tiles_y;
    int b0, nb;
    if (row) bg_block(i * a.tile, a.tile, a.height, a.sy, a.Hg, &b0, &nb);
    else bg_block(i * a.tile, a.tile, a.width, a.sx, a.Wg, &b0, &nb);
    const int node = row ? y : x;
    if (node >= b0 && node < b0 + nb) {
      atomicMin(&s_range[row ? 0 : 2], i);
      atomicMax(&s_range[row ? 1 : 3], i);
    }
  }
  __syncthreads();
  const int ty0 = s_range[0], my = s_range[1] - ty0 + 1, tx0 = s_range[2], mx = s_range[3] - tx0 + 1;
  const int members = (my > 0 && mx > 0) ? my * mx : 0;  // a grid finer than the image has nodes no pixel touches
  const int c = tid % BG_CH, slice = tid / BG_CH;
  if (slice < BG_FIN_SLICES) {
    double sum = 0.0;
    for (int m = slice; m < members; m += BG_FIN_SLICES) {
      const int ty = ty0 + m / mx, tx = tx0 + m % mx;
      int by0, nby, bx0, nbx;
      bg_block(ty * a.tile, a.tile, a.height, a.sy, a.Hg, &by0, &nby);
      bg_block(tx * a.tile, a.tile, a.width, a.sx, a.Wg, &bx0, &nbx);
      const int64_t slot = (int64_t(b) * a.tiles_y + ty) * a.tiles_x + tx;
      sum += double(a.partials[slot * a.block_elems + ((z * nby + (y - by0)) * nbx + (x - bx0)) * BG_CH + c]);
    }
    s_part[slice][c] = sum;
  }
  __syncthreads();
  if (tid < BG_CH) {
    double sum = 0.0;
    for (int i = 0; i < BG_FIN_SLICES; ++i) sum += s_part[i][tid];
    d_grid[((int64_t(b) * BG_CH + tid) * a.L + z) * a.Hg * a.Wg + int64_t(y) * a.Wg + x] = T(sum);
  }
}

// ------------------------------------------------------------------------------------------------------------- host
struct BgPlan {
  int tile, tile_shift, tiles_x, tiles_y, block_elems;
  int64_t groups;
};

template <typename T>
int bg_max_nodes(int extent, int tile, T scale, int size) {
  int most = 0;
  for (int t0 = 0; t0 < extent; t0 += tile) {
    int b0, nb;
    bg_block(t0, tile, extent, scale, size, &b0, &nb);
    most = nb > most ? nb : most;
  }
  return most;
}

template <typename T>
T bg_scale(int64_t size, int64_t extent) { return T(double(size - 1) / double(extent)); }

int bg_sizes(const char* who, int64_t batch, int64_t height, int64_t width, int64_t L, int64_t Hg, int64_t Wg) {
  GS_REQUIRE(batch > 0 && height > 0 && width > 0, GS_ERR_INVALID_ARGUMENT, "%s: image %lld x %lld x %lld is empty", who,
             (long long)batch, (long long)height, (long long)width);
  GS_REQUIRE(L > 0 && Hg > 0 && Wg > 0, GS_ERR_INVALID_ARGUMENT, "%s: grid size %lld x %lld x %lld", who, (long long)L,
             (long long)Hg, (long long)Wg);
  GS_REQUIRE(height <= (1 << 22) && width <= (1 << 22), GS_ERR_UNSUPPORTED,
             "%s: image %lld x %lld above 4194304 pixels a side", who, (long long)height, (long long)width);
  GS_REQUIRE(L <= (1 << 20) && Hg <= (1 << 20) && Wg <= (1 << 20) && BG_CH * L * Hg * Wg < (int64_t(1) << 31),
             GS_ERR_UNSUPPORTED, "%s: grid %lld x %lld x %lld above 2^31 elements", who, (long long)L, (long long)Hg,
             (long long)Wg);
  return GS_OK;
}

// the tile edge: the largest whose blocks fit (a smaller tile never touches more nodes) and, above 8, which leaves
// BG_MIN_GROUPS workgroups.  A one-pixel tile touches 2 x 2 x L nodes: only L can be too large.
template <typename T>
int bg_plan(const char* who, int64_t batch, int64_t height, int64_t width, int64_t L, int64_t Hg, int64_t Wg,
            BgPlan* plan) {
  const int max_elems = BG_LDS_BYTES / (2 * int(sizeof(T)));
  const T sx = bg_scale<T>(Wg, width), sy = bg_scale<T>(Hg, height);
  int found = -1, elems[BG_NUM_TILES];
  for (int i = 0; i < BG_NUM_TILES && found < 0; ++i) {
    const int tile = BG_TILES[i];
    const int64_t nodes = int64_t(bg_max_nodes(int(width), tile, sx, int(Wg))) *
                          bg_max_nodes(int(height), tile, sy, int(Hg));
    const int64_t n = nodes * L * BG_CH;
    if (n > max_elems) continue;
    elems[i] = int(n);
    const int64_t groups = batch * gs_div_up(width, tile) * gs_div_up(height, tile);
    if (tile <= 8 || groups >= BG_MIN_GROUPS) found = i;
  }
  GS_REQUIRE(found >= 0, GS_ERR_UNSUPPORTED,
             "%s: L = %lld: the 2 x 2 x L x 12 nodes of one pixel must fit in %d bytes of LDS twice (L <= %d)", who,
             (long long)L, BG_LDS_BYTES, max_elems / (4 * BG_CH));
  const int tile = BG_TILES[found];
  plan->tile = tile;
  plan->tile_shift = 0;
  while ((1 << plan->tile_shift) < tile) ++plan->tile_shift;
  plan->tiles_x = int(gs_div_up(width, tile));
  plan->tiles_y = int(gs_div_up(height, tile));
  plan->block_elems = elems[found];
  plan->groups = batch * plan->tiles_x * plan->tiles_y;
  GS_REQUIRE(plan->groups < (int64_t(1) << 31), GS_ERR_UNSUPPORTED, "%s: %lld pixel tiles above the launch limit 2^31",
             who, (long long)plan->groups);
  return GS_OK;
}

template <typename T>
int bg_image(const char* who, const char* name, int channels, int64_t batch, int64_t height, int64_t width, const T* p,
             int64_t sb, int64_t sr, int64_t sp, BgImage<T>* out) {
  GS_REQUIRE(sp >= channels && sr >= width * sp && (batch <= 1 || sb >= height * sr), GS_ERR_INVALID_ARGUMENT,
             "%s: bad strides of %s (batch %lld, row %lld, pixel %lld elements for %lld x %lld x %d)", who, name,
             (long long)sb, (long long)sr, (long long)sp, (long long)height, (long long)width, channels);
  out->p = p; out->sb = sb; out->sr = sr; out->sp = sp;
  return GS_OK;
}

// what both directions check and fill alike
template <typename T>
int bg_common(const char* who, int64_t batch, int64_t height, int64_t width, const T* image, int64_t isb, int64_t isr,
              int64_t isp, const T* guide, int64_t gsb, int64_t gsr, int64_t gsp, const T* grid, int64_t L, int64_t Hg,
              int64_t Wg, int64_t grid_sb, BgArgs<T>* a, BgPlan* plan) {
  GS_TRY(bg_sizes(who, batch, height, width, L, Hg, Wg));
  GS_REQUIRE(image != nullptr && grid != nullptr, GS_ERR_INVALID_ARGUMENT, "%s: NULL buffer (image / grid)", who);
  GS_TRY(bg_image(who, "image", 3, batch, height, width, image, isb, isr, isp, &a->x));
  a->guide = BgImage<T>{nullptr, 0, 0, 0};
  if (guide) GS_TRY(bg_image(who, "guide", 1, batch, height, width, guide, gsb, gsr, gsp, &a->guide));
  GS_REQUIRE(batch <= 1 || grid_sb >= BG_CH * L * Hg * Wg, GS_ERR_INVALID_ARGUMENT,
             "%s: grid batch stride %lld below the %lld elements of one grid", who, (long long)grid_sb,
             (long long)(BG_CH * L * Hg * Wg));
  GS_TRY(bg_plan<T>(who, batch, height, width, L, Hg, Wg, plan));
  a->batch = int(batch); a->height = int(height); a->width = int(width);
  a->L = int(L); a->Hg = int(Hg); a->Wg = int(Wg);
  a->tile = plan->tile; a->tile_shift = plan->tile_shift; a->tiles_x = plan->tiles_x; a->tiles_y = plan->tiles_y;
  a->block_elems = plan->block_elems;
  a->sx = bg_scale<T>(Wg, width); a->sy = bg_scale<T>(Hg, height); a->sz = T(L - 1);
  a->grid = grid; a->grid_sb = grid_sb;
  a->out = nullptr; a->grad_out = nullptr; a->d_image = nullptr; a->d_guide = nullptr; a->partials = nullptr;
  return GS_OK;
}

template <typename T>
int bg_fwd(const char* who, int64_t batch, int64_t height, int64_t width, const T* image, int64_t isb, int64_t isr,
           int64_t isp, const T* guide, int64_t gsb, int64_t gsr, int64_t gsp, const T* grid, int64_t L, int64_t Hg,
           int64_t Wg, int64_t grid_sb, T* out, void* stream) {
  BgArgs<T> a;
  BgPlan plan;
  GS_TRY(bg_common(who, batch, height, width, image, isb, isr, isp, guide, gsb, gsr, gsp, grid, L, Hg, Wg, grid_sb, &a,
                   &plan));
  GS_REQUIRE(out != nullptr, GS_ERR_INVALID_ARGUMENT, "%s: NULL buffer (out)", who);
  a.out = out;
  const size_t lds = size_t(plan.block_elems) * sizeof(T);
  hipLaunchKernelGGL(bilagrid_fwd_kernel<T>, dim3(unsigned(plan.groups)), dim3(GS_WAVE), lds,
                     static_cast<hipStream_t>(stream), a);
  GS_CHECK_LAUNCH(who);
  return GS_OK;
}

template <typename T>
int64_t bg_scratch_bytes(const BgPlan& plan) { return plan.groups * plan.block_elems * int64_t(sizeof(T)); }

template <typename T>
int bg_bwd(const char* who, int64_t batch, int64_t height, int64_t width, const T* image, int64_t isb, int64_t isr,
           int64_t isp, const T* guide, int64_t gsb, int64_t gsr, int64_t gsp, const T* grid, int64_t L, int64_t Hg,
           int64_t Wg, int64_t grid_sb, const T* grad_out, T* d_image, T* d_guide, T* d_grid, void* scratch,
           int64_t scratch_bytes, void* stream) {
  BgArgs<T> a;
  BgPlan plan;
  GS_TRY(bg_common(who, batch, height, width, image, isb, isr, isp, guide, gsb, gsr, gsp, grid, L, Hg, Wg, grid_sb, &a,
                   &plan));
  GS_REQUIRE(grad_out != nullptr, GS_ERR_INVALID_ARGUMENT, "%s: NULL buffer (grad_out)", who);
  GS_REQUIRE(d_image || d_guide || d_grid, GS_ERR_INVALID_ARGUMENT, "%s: NULL buffer (no gradient asked for)", who);
  GS_REQUIRE(!d_guide || guide, GS_ERR_INVALID_ARGUMENT, "%s: d_guide without a guide", who);
  if (d_grid) {
    GS_REQUIRE(batch * L * Hg * Wg < (int64_t(1) << 31), GS_ERR_UNSUPPORTED,
               "%s: %lld grid nodes above the launch limit 2^31", who, (long long)(batch * L * Hg * Wg));
    GS_TRY(gs_check_scratch(who, scratch, scratch_bytes, bg_scratch_bytes<T>(plan)));
    a.partials = static_cast<T*>(scratch);
  }
  a.grad_out = grad_out; a.d_image = d_image; a.d_guide = d_guide;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t lds = 2 * size_t(plan.block_elems) * sizeof(T);
  hipLaunchKernelGGL(bilagrid_bwd_kernel<T>, dim3(unsigned(plan.groups)), dim3(GS_WAVE), lds, st, a);
  GS_CHECK_LAUNCH(who);
  if (d_grid) {
    hipLaunchKernelGGL(bilagrid_finish_kernel<T>, dim3(unsigned(batch * L * Hg * Wg)), dim3(BG_FIN_THREADS), 0, st, a,
                       d_grid);
    GS_CHECK_LAUNCH(who);
  }
  return GS_OK;
}

}  // namespace

extern "C" int64_t gs_bilagrid_scratch_bytes(int64_t batch, int64_t height, int64_t width, int64_t grid_l,
                                              int64_t grid_h, int64_t grid_w, int32_t f64) {
  const char* who = "gs_bilagrid_scratch_bytes";
  BgPlan plan;
  GS_TRY(bg_sizes(who, batch, height, width, grid_l, grid_h, grid_w));
  if (f64) {
    GS_TRY(bg_plan<double>(who, batch, height, width, grid_l, grid_h, grid_w, &plan));
    return bg_scratch_bytes<double>(plan);
  }
  GS_TRY(bg_plan<float>(who, batch, height, width, grid_l, grid_h, grid_w, &plan));
  return bg_scratch_bytes<float>(plan);
}

extern "C" int gs_bilagrid_slice_fwd(int64_t batch, int64_t height, int64_t width, const float* image,
                                     int64_t image_batch_stride, int64_t image_row_stride, int64_t image_pixel_stride,
                                     const float* guide, int64_t guide_batch_stride, int64_t guide_row_stride,
                                     int64_t guide_pixel_stride, const float* grid, int64_t grid_l, int64_t grid_h,
                                     int64_t grid_w, int64_t grid_batch_stride, float* out, void* stream) {
  return bg_fwd<float>("gs_bilagrid_slice_fwd", batch, height, width, image, image_batch_stride, image_row_stride,
                       image_pixel_stride, guide, guide_batch_stride, guide_row_stride, guide_pixel_stride, grid,
                       grid_l, grid_h, grid_w, grid_batch_stride, out, stream);
}

extern "C" int gs_bilagrid_slice_fwd_f64(int64_t batch, int64_t height, int64_t width, const double* image,
                                         int64_t image_batch_stride, int64_t image_row_stride,
                                         int64_t image_pixel_stride, const double* guide, int64_t guide_batch_stride,
                                         int64_t guide_row_stride, int64_t guide_pixel_stride, const double* grid,
                                         int64_t grid_l, int64_t grid_h, int64_t grid_w, int64_t grid_batch_stride,
                                         double* out, void* stream) {
  return bg_fwd<double>("gs_bilagrid_slice_fwd_f64", batch, height, width, image, image_batch_stride, image_row_stride,
                        image_pixel_stride, guide, guide_batch_stride, guide_row_stride, guide_pixel_stride, grid,
                        grid_l, grid_h, grid_w, grid_batch_stride, out, stream);
}

extern "C" int gs_bilagrid_slice_bwd(int64_t batch, int64_t height, int64_t width, const float* image,
                                     int64_t image_batch_stride, int64_t image_row_stride, int64_t image_pixel_stride,
                                     const float* guide, int64_t guide_batch_stride, int64_t guide_row_stride,
                                     int64_t guide_pixel_stride, const float* grid, int64_t grid_l, int64_t grid_h,
                                     int64_t grid_w, int64_t grid_batch_stride, const float* grad_out, float* d_image,
                                     float* d_guide, float* d_grid, void* scratch, int64_t scratch_bytes,
                                     void* stream) {
  return bg_bwd<float>("gs_bilagrid_slice_bwd", batch, height, width, image, image_batch_stride, image_row_stride,
                       image_pixel_stride, guide, guide_batch_stride, guide_row_stride, guide_pixel_stride, grid,
                       grid_l, grid_h, grid_w, grid_batch_stride, grad_out, d_image, d_guide, d_grid, scratch,
                       scratch_bytes, stream);
}

extern "C" int gs_bilagrid_slice_bwd_f64(int64_t batch, int64_t height, int64_t width, const double* image,
                                         int64_t image_batch_stride, int64_t image_row_stride,
                                         int64_t image_pixel_stride, const double* guide, int64_t guide_batch_stride,
                                         int64_t guide_row_stride, int64_t guide_pixel_stride, const double* grid,
                                         int64_t grid_l, int64_t grid_h, int64_t grid_w, int64_t grid_batch_stride,
                                         const double* grad_out, double* d_image, double* d_guide, double* d_grid,
                                         void* scratch, int64_t scratch_bytes, void* stream) {
  return bg_bwd<double>("gs_bilagrid_slice_bwd_f64", batch, height, width, image, image_batch_stride, image_row_stride,
                        image_pixel_stride, guide, guide_batch_stride, guide_row_stride, guide_pixel_stride, grid,
                        grid_l, grid_h, grid_w, grid_batch_stride, grad_out, d_image, d_guide, d_grid, scratch,
                        scratch_bytes, stream);
}
