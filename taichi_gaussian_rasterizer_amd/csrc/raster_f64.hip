// raster_f64.hip -- the tile rasterizer and its adjoint in float64, for gradcheck.  Reference:
// rasterizer/forward.py:25-137, rasterizer/backward.py:53-228, taichi_lib/generic.py:311-336 (gaussian_pdf and its
// gradient), :341-404 (antialias variants).  The spec is the f64 oracle (oracle/gsplat_oracle.cpp raster_fwd /
// raster_bwd), which restates those formulas.
//
// The reference formulas literally, in IEEE double: none of the f32 kernels' reformulations (no ellipse frame, no
// exp2 fast math, no clamp of the antialias sigmoid's argument, no early stop of the forward: forward_cut does not
// exist here).  One workgroup per tile, one pixel per lane; a tile's list is staged through LDS in batches of BATCH
// splats.  Deterministic: each (tile, list entry k) writes its own record -- the visibility in the forward, the 7 + F + 2
// gradient values in the backward -- with plain stores after a fixed-order workgroup sum; every splat then adds its
// records in ascending k (f64_common.h gs_f64_group).  The tile ranges must be disjoint, as the mapper makes them.

#include "f64_common.h"

namespace {

constexpr int BATCH = 32;
constexpr double TAU = 2.0 * 3.14159265358979323846;

struct Cfg {
  int antialias, blend;
  double cmax, thr, sat;  // sat: the backward's saturate_threshold, the forward's quantile level 1 - threshold
};

// generic.py:311-336
__device__ __forceinline__ double pdf_plain(double px, double py, const double* g) {
  const double dx = px - g[0], dy = py - g[1];
  const double tx = (dx * g[2] + dy * g[3]) / g[4];
  const double ty = (dx * -g[3] + dy * g[2]) / g[5];
  return exp(-0.5 * (tx * tx + ty * ty));
}

__device__ __forceinline__ double pdf_plain_grad(double px, double py, const double* g, double dmean[2],
                                                 double daxis[2], double dsigma[2]) {
  const double dx = px - g[0], dy = py - g[1];
  const double ax = g[2], ay = g[3], sx = g[4], sy = g[5];
  const double tx = (dx * ax + dy * ay) / sx;
  const double ty = (dx * -ay + dy * ax) / sy;
  const double tx2 = tx * tx, ty2 = ty * ty;
  const double p = exp(-0.5 * (tx2 + ty2));
  dsigma[0] = tx2 * p / sx;
  dsigma[1] = ty2 * p / sy;
  const double txs = tx / sx, tys = ty / sy;
  daxis[0] = p * (txs * -dx + tys * -dy);
  daxis[1] = p * (txs * -dy + tys * dx);
  dmean[0] = p * (txs * ax + tys * -ay);
  dmean[1] = p * (txs * ay + tys * ax);
  return p;
}

// generic.py:341-404: the pixel's integral of a logistic approximation of the normal cdf, S(t + 1/2) - S(t - 1/2)
__device__ __forceinline__ double s_sig(double x, double sigma) {
  const double z = x / sigma;
  return 1.0 / (1.0 + exp(-1.6 * z - 0.07 * z * z * z));
}

__device__ __forceinline__ void s_sig_grad(double x, double sigma, double& s, double& ds_dx, double& ds_dsig) {
  const double z = x / sigma;
  s = 1.0 / (1.0 + exp(-1.6 * z - 0.07 * z * z * z));
  const double d = (1.6 + 0.21 * z * z) * s * (1.0 - s);
  ds_dx = d / sigma;
  ds_dsig = ds_dx * -z;
}

__device__ __forceinline__ double pdf_aa(double px, double py, const double* g) {
  const double dx = px - g[0], dy = py - g[1];
  const double sx = g[4], sy = g[5];
  const double tx = dx * g[2] + dy * g[3];
  const double ty = dx * -g[3] + dy * g[2];
  const double Sx1 = s_sig(tx + 0.5, sx), Sx2 = s_sig(tx - 0.5, sx);
  const double Sy1 = s_sig(ty + 0.5, sy), Sy2 = s_sig(ty - 0.5, sy);
  return TAU * sx * (Sx1 - Sx2) * sy * (Sy1 - Sy2);
}

__device__ __forceinline__ double pdf_aa_grad(double px, double py, const double* g, double dmean[2], double daxis[2],
                                              double dsigma[2]) {
  const double dx = px - g[0], dy = py - g[1];
  const double ax = g[2], ay = g[3], sx = g[4], sy = g[5];
  const double tx = dx * ax + dy * ay;
  const double ty = dx * -ay + dy * ax;
  double Sx1, dSx1, dSx1s, Sx2, dSx2, dSx2s, Sy1, dSy1, dSy1s, Sy2, dSy2, dSy2s;
  s_sig_grad(tx + 0.5, sx, Sx1, dSx1, dSx1s);
  s_sig_grad(tx - 0.5, sx, Sx2, dSx2, dSx2s);
  s_sig_grad(ty + 0.5, sy, Sy1, dSy1, dSy1s);
  s_sig_grad(ty - 0.5, sy, Sy2, dSy2, dSy2s);
  const double ix = sx * (Sx1 - Sx2), iy = sy * (Sy1 - Sy2);
  const double dSx = iy * sx * (dSx1 - dSx2);
  const double dSy = ix * sy * (dSy1 - dSy2);
  dmean[0] = TAU * (dSx * -ax + dSy * ay);
  dmean[1] = TAU * (dSx * -ay + dSy * -ax);
  dsigma[0] = TAU * iy * (Sx1 - Sx2 + (dSx1s - dSx2s) * sx);
  dsigma[1] = TAU * ix * (Sy1 - Sy2 + (dSy1s - dSy2s) * sy);
  daxis[0] = TAU * (dSx * dx + dSy * dy);
  daxis[1] = TAU * (dSx * dy + dSy * -dx);
  return TAU * ix * iy;
}

// Stage list entries [base, base + nb) of the tile: splat rows and their features.  An entry naming no splat of
// [0, v) stages a zero row (alpha 0: it never blends).
template <int NT, int FM>
__device__ __forceinline__ void stage(int base, int nb, int64_t v, int F, const double* points, const double* features,
                                      const int32_t* o2p, double (*s_g)[7], double (*s_f)[FM]) {
  for (int e = threadIdx.x; e < nb * 7; e += NT) {
    const int j = e / 7, r = e - j * 7;
    const int idx = o2p[base + j];
    s_g[j][r] = (idx >= 0 && idx < v) ? points[int64_t(idx) * 7 + r] : 0.0;
  }
  for (int e = threadIdx.x; e < nb * F; e += NT) {
    const int j = e / F, r = e - j * F;
    const int idx = o2p[base + j];
    s_f[j][r] = (idx >= 0 && idx < v) ? features[int64_t(idx) * F + r] : 0.0;
  }
}

struct TileArgs {
  int64_t v, k;
  int F, width, height, tiles_x;
  const double* points;
  const double* features;
  const int32_t* ranges;
  const int32_t* o2p;
  Cfg c;
  // optional (raster_fwd.hip / raster_bwd.hip): the forward's background of channels [bg_off, F); the backward's alpha
  // image and gradient of the weight image
  const double* bg;
  const double* alpha_in;
  const double* grad_weight;
  int bg_off;
};

// the tile's list [start, end), clamped to [0, k)
__device__ __forceinline__ void tile_list(const TileArgs& a, int& start, int& end) {
  const int64_t s = a.ranges[2 * blockIdx.x], e = a.ranges[2 * blockIdx.x + 1];
  start = int(s < 0 ? 0 : (s > a.k ? a.k : s));
  end = int(e < start ? start : (e > a.k ? a.k : e));
}

// rasterizer/forward.py:84-128, as the oracle reads it: blend the whole list (alpha blending), or stop at the entry
// that takes the accumulated alpha past 1 - saturate_threshold and take its features (quantile mode).
template <int TS, int FM>
__global__ __launch_bounds__(TS * TS) void raster_fwd_f64_kernel(TileArgs a, double* image, double* alpha_img,
                                                                 double* vis_rec) {
  constexpr int NT = TS * TS, NW = NT / 64;
  __shared__ double s_g[BATCH][7];
  __shared__ double s_f[BATCH][FM];
  __shared__ double s_w[BATCH][NW];
  const int px = (int(blockIdx.x) % a.tiles_x) * TS + int(threadIdx.x) % TS;
  const int py = (int(blockIdx.x) / a.tiles_x) * TS + int(threadIdx.x) / TS;
  const bool inside = px < a.width && py < a.height;
  const double pxf = double(px) + 0.5, pyf = double(py) + 0.5;
  int start, end;
  tile_list(a, start, end);
  const Cfg& c = a.c;
  double acc[FM];
#pragma unroll
  for (int ch = 0; ch < FM; ++ch) acc[ch] = 0.0;
  double total = 0.0;
  bool done = !inside;
  for (int base = start; base < end; base += BATCH) {
    const int nb = min(BATCH, end - base);
    __syncthreads();  // the previous batch is consumed
    stage<NT, FM>(base, nb, a.v, a.F, a.points, a.features, a.o2p, s_g, s_f);
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
      double w = 0.0;
      if (!done) {
        const double ga = c.antialias ? pdf_aa(pxf, pyf, s_g[j]) : pdf_plain(pxf, pyf, s_g[j]);
        double al = s_g[j][6] * ga;
        if (c.cmax < al) al = c.cmax;  // forward.py:99
        if (al > c.thr) {
          w = al * (1.0 - total);
          total += w;
          if (c.blend) {
#pragma unroll
            for (int ch = 0; ch < FM; ++ch)
              if (ch < a.F) acc[ch] += s_f[j][ch] * w;
          } else if (total >= c.sat) {  // forward.py:109-114
#pragma unroll
            for (int ch = 0; ch < FM; ++ch)
              if (ch < a.F) acc[ch] = s_f[j][ch];
            done = true;
          }
        }
      }
      if (vis_rec) {
        const double s = gs_f64_wave_sum(w);
        if ((threadIdx.x & 63) == 0) s_w[j][threadIdx.x >> 6] = s;
      }
    }
    if (vis_rec) {
      __syncthreads();
      if (int(threadIdx.x) < nb) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += s_w[threadIdx.x][w];
        vis_rec[base + threadIdx.x] = t;
      }
    }
  }
  if (inside) {
    double* out = image + (int64_t(py) * a.width + px) * a.F;
    if (a.bg != nullptr) {  // composite on the background with the final transmittance
#pragma unroll
      for (int ch = 0; ch < FM; ++ch)
        if (ch >= a.bg_off && ch < a.F) acc[ch] += (1.0 - total) * a.bg[ch - a.bg_off];
    }
#pragma unroll
    for (int ch = 0; ch < FM; ++ch)
      if (ch < a.F) out[ch] = acc[ch];
    alpha_img[int64_t(py) * a.width + px] = c.blend ? total : (total > 0.0 ? 1.0 : 0.0);
  }
}

// rasterizer/backward.py:140-198 front to back, as the oracle reads it: the remaining colour starts at the forward's
// image and loses each blended splat's share.  Record of entry k: [d(mean, axis, sigma, alpha), d(features),
// heuristics], 7 + F + 2 doubles.
template <int TS, int FM>
__global__ __launch_bounds__(TS * TS) void raster_bwd_f64_kernel(TileArgs a, const double* image,
                                                                 const double* grad_image, double* rec) {
  constexpr int NT = TS * TS, NW = NT / 64, RM = 7 + FM + 2;
  __shared__ double s_g[BATCH][7];
  __shared__ double s_f[BATCH][FM];
  __shared__ double s_part[2][NW][RM];
  const int px = (int(blockIdx.x) % a.tiles_x) * TS + int(threadIdx.x) % TS;
  const int py = (int(blockIdx.x) / a.tiles_x) * TS + int(threadIdx.x) / TS;
  const bool inside = px < a.width && py < a.height;
  const double pxf = double(px) + 0.5, pyf = double(py) + 0.5;
  const int F = a.F, R = 7 + F + 2;
  int start, end;
  tile_list(a, start, end);
  const Cfg& c = a.c;
  const int64_t pix = inside ? int64_t(py) * a.width + px : 0;
  const double* gpix = grad_image + pix * F;
  double rem[FM];
#pragma unroll
  for (int ch = 0; ch < FM; ++ch) rem[ch] = (inside && ch < F) ? image[pix * F + ch] : 0.0;
  // the weight image's gradient: the background acts as a last splat of opacity 1, and the weight as one more channel
  // whose "background" is -1 (weight = 1 - T): its remaining colour is -T g_W from the first splat to the last
  const bool weight_grad = a.grad_weight != nullptr;
  const double rem_w = (weight_grad && inside) ? (a.alpha_in[pix] - 1.0) * a.grad_weight[pix] : 0.0;
  double total = 0.0;
  bool done = !inside;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int buf = 0;
  for (int base = start; base < end; base += BATCH) {
    const int nb = min(BATCH, end - base);
    __syncthreads();
    stage<NT, FM>(base, nb, a.v, F, a.points, a.features, a.o2p, s_g, s_f);
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
      bool hit = false;
      double dmean[2] = {0, 0}, daxis[2] = {0, 0}, dsigma[2] = {0, 0}, ga = 0.0, alpha_grad = 0.0, w = 0.0;
      if (!done && total >= c.sat) done = true;  // backward.py:160
      if (!done) {
        const double* g = s_g[j];
        ga = c.antialias ? pdf_aa_grad(pxf, pyf, g, dmean, daxis, dsigma)
                         : pdf_plain_grad(pxf, pyf, g, dmean, daxis, dsigma);
        double al = g[6] * ga;
        if (al > c.thr) {  // backward.py:166 (unclamped alpha)
          hit = true;
          if (c.cmax < al) al = c.cmax;  // :169
          const double Ti = 1.0 - total;
          w = al * Ti;
          total += w;
#pragma unroll
          for (int ch = 0; ch < FM; ++ch)
            if (ch < F) {
              rem[ch] -= s_f[j][ch] * w;
              const double diff = s_f[j][ch] * Ti - rem[ch] / (1.0 - al);  // :180
              alpha_grad += diff * gpix[ch];
            }
          if (weight_grad) alpha_grad -= rem_w / (1.0 - al);
        }
      }
      const double aag = s_g[j][6] * alpha_grad;  // :184
      double* part = s_part[buf][wave];
      if (__any(hit)) {
        // lanes that blend nothing add exact zeros (not 0 * a pdf gradient, which may be inf far from the centre)
        const double vals[9] = {hit ? aag * dmean[0] : 0.0, hit ? aag * dmean[1] : 0.0, hit ? aag * daxis[0] : 0.0,
                                hit ? aag * daxis[1] : 0.0, hit ? aag * dsigma[0] : 0.0, hit ? aag * dsigma[1] : 0.0,
                                hit ? ga * alpha_grad : 0.0, hit ? aag * aag : 0.0,
                                hit ? fabs(aag * dmean[0]) + fabs(aag * dmean[1]) : 0.0};
#pragma unroll
        for (int r = 0; r < 7; ++r) {
          const double s = gs_f64_wave_sum(vals[r]);
          if (lane == 0) part[r] = s;
        }
#pragma unroll
        for (int ch = 0; ch < FM; ++ch)
          if (ch < F) {
            const double s = gs_f64_wave_sum(hit ? w * gpix[ch] : 0.0);
            if (lane == 0) part[7 + ch] = s;
          }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const double s = gs_f64_wave_sum(vals[7 + r]);
          if (lane == 0) part[7 + F + r] = s;
        }
      } else if (lane < R) {
        part[lane] = 0.0;
      }
      __syncthreads();
      // one barrier per entry: the next entry writes the other half of s_part
      if (int(threadIdx.x) < R) {
        double t = 0.0;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) t += s_part[buf][ww][threadIdx.x];
        rec[int64_t(base + j) * R + threadIdx.x] = t;
      }
      buf ^= 1;
    }
  }
}

// every splat adds its records in ascending k: columns [0, na) of a record go to a, [na, na + nb) to b, the rest to c
// (which may be NULL)
__global__ __launch_bounds__(256) void sum_records_kernel(int64_t v, int R, const double* rec, const int32_t* order,
                                                          const int32_t* seg, double* a, int na, double* b, int nb,
                                                          double* c) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= v) return;
  const int e0 = seg[2 * i], e1 = seg[2 * i + 1];
  for (int r = 0; r < R; ++r) {
    double t = 0.0;
    for (int e = e0; e < e1; ++e) t += rec[int64_t(order[e]) * R + r];
    if (r < na) a[i * na + r] = t;
    else if (r < na + nb) b[i * nb + (r - na)] = t;
    else if (c) c[i * (R - na - nb) + (r - na - nb)] = t;
  }
}

__global__ __launch_bounds__(256) void iota_kernel(int64_t k, int32_t* out) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i < k) out[i] = int32_t(i);
}

template <typename K>
__global__ __launch_bounds__(256) void segments_kernel(int64_t k, const K* sk, int64_t n, int32_t* seg) {
  const int64_t p = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (p >= k) return;
  const K key = sk[p];
  if (key >= K(n)) return;  // unsigned: negative keys are out of range too
  if (p == 0 || sk[p - 1] != key) seg[2 * key] = int32_t(p);
  if (p == k - 1 || sk[p + 1] != key) seg[2 * key + 1] = int32_t(p + 1);
}

int64_t records(int64_t k, int32_t num_features) { return gs_align_up((k > 0 ? k : 1) * (9 + num_features) * 8, 256); }

int check_raster(int64_t v, int32_t F, const double* points, const double* features, const int32_t* tile_ranges,
                 const int32_t* o2p, int64_t k, int32_t width, int32_t height, const GsRasterConfigF64* cfg,
                 const void* out0, const void* out1, void* scratch, int64_t scratch_bytes, const char* what) {
  GS_REQUIRE(cfg != nullptr, GS_ERR_INVALID_ARGUMENT, "%s: config is NULL", what);
  GS_REQUIRE(cfg->tile_size == 8 || cfg->tile_size == 16 || cfg->tile_size == 32, GS_ERR_UNSUPPORTED,
             "%s: tile_size %d not supported (8, 16 or 32)", what, cfg->tile_size);
  GS_REQUIRE(F >= 1 && F <= GS_MAX_FEATURES, GS_ERR_UNSUPPORTED,
             "%s: feature width %d not supported (1 to %d in float64)", what, F, GS_MAX_FEATURES);
  GS_REQUIRE(cfg->alpha_threshold > 0.0, GS_ERR_INVALID_ARGUMENT, "%s: alpha_threshold must be > 0", what);
  GS_REQUIRE(v >= 0 && v < (int64_t(1) << 31) && k >= 0 && k < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT,
             "%s: %lld splats, %lld list entries", what, (long long)v, (long long)k);
  GS_REQUIRE(width > 0 && height > 0, GS_ERR_INVALID_ARGUMENT, "%s: image size %dx%d", what, width, height);
  GS_REQUIRE(tile_ranges && out0 && out1 && (v == 0 || (points && features)) && (k == 0 || o2p),
             GS_ERR_INVALID_ARGUMENT, "%s: NULL buffer", what);
  GS_REQUIRE(scratch && scratch_bytes >= gs_raster_f64_scratch_bytes(v, k, F), GS_ERR_SCRATCH_TOO_SMALL,
             "%s: scratch %lld < %lld", what, (long long)scratch_bytes, (long long)gs_raster_f64_scratch_bytes(v, k, F));
  return GS_OK;
}

TileArgs tile_args(int64_t v, int32_t F, const double* points, const double* features, const int32_t* tile_ranges,
                   const int32_t* o2p, int64_t k, int32_t width, int32_t height, const GsRasterConfigF64* cfg,
                   bool forward) {
  TileArgs a;
  a.v = v; a.k = k; a.F = F; a.width = width; a.height = height;
  a.tiles_x = int(gs_div_up(width, cfg->tile_size));
  a.points = points; a.features = features; a.ranges = tile_ranges; a.o2p = o2p;
  a.c.antialias = cfg->antialias != 0;
  a.c.blend = cfg->use_alpha_blending != 0;
  a.c.cmax = cfg->clamp_max_alpha;
  a.c.thr = cfg->alpha_threshold;
  a.c.sat = forward ? 1.0 - cfg->saturate_threshold : cfg->saturate_threshold;
  a.bg = a.alpha_in = a.grad_weight = nullptr;
  a.bg_off = 0;
  return a;
}

template <int TS, int FM>
void launch_fwd(int tiles, const TileArgs& a, double* image, double* alpha, double* vis_rec, hipStream_t s) {
  hipLaunchKernelGGL((raster_fwd_f64_kernel<TS, FM>), dim3(tiles), dim3(TS * TS), 0, s, a, image, alpha, vis_rec);
}

template <int TS, int FM>
void launch_bwd(int tiles, const TileArgs& a, const double* image, const double* grad_image, double* rec,
                hipStream_t s) {
  hipLaunchKernelGGL((raster_bwd_f64_kernel<TS, FM>), dim3(tiles), dim3(TS * TS), 0, s, a, image, grad_image, rec);
}

template <int TS>
void dispatch_fwd(int tiles, const TileArgs& a, double* image, double* alpha, double* vis_rec, hipStream_t s) {
  if (a.F <= 4) launch_fwd<TS, 4>(tiles, a, image, alpha, vis_rec, s);
  else if (a.F <= 8) launch_fwd<TS, 8>(tiles, a, image, alpha, vis_rec, s);
  else if (a.F <= 16) launch_fwd<TS, 16>(tiles, a, image, alpha, vis_rec, s);
  else launch_fwd<TS, 32>(tiles, a, image, alpha, vis_rec, s);
}

template <int TS>
void dispatch_bwd(int tiles, const TileArgs& a, const double* image, const double* grad_image, double* rec,
                  hipStream_t s) {
  if (a.F <= 4) launch_bwd<TS, 4>(tiles, a, image, grad_image, rec, s);
  else if (a.F <= 8) launch_bwd<TS, 8>(tiles, a, image, grad_image, rec, s);
  else if (a.F <= 16) launch_bwd<TS, 16>(tiles, a, image, grad_image, rec, s);
  else launch_bwd<TS, 32>(tiles, a, image, grad_image, rec, s);
}

}  // namespace

int64_t gs_f64_group_scratch_bytes(int64_t k, int64_t n, int key_bytes) {
  return gs_align_up(k * 4, 256) * 2 + gs_align_up(k * key_bytes, 256) + gs_align_up((n > 0 ? n : 1) * 8, 256) +
         gs_sort_scratch_bytes(k, key_bytes);
}

int gs_f64_group(int64_t k, int key_bytes, const void* keys, int64_t n, int32_t** order, int32_t** seg, void* scratch,
                 int64_t scratch_bytes, hipStream_t s) {
  GS_REQUIRE(scratch_bytes >= gs_f64_group_scratch_bytes(k, n, key_bytes), GS_ERR_SCRATCH_TOO_SMALL,
             "float64 grouping: scratch too small");
  char* p = static_cast<char*>(scratch);
  int32_t* iota = reinterpret_cast<int32_t*>(p);
  p += gs_align_up(k * 4, 256);
  *order = reinterpret_cast<int32_t*>(p);
  p += gs_align_up(k * 4, 256);
  void* sorted_keys = p;
  p += gs_align_up(k * key_bytes, 256);
  *seg = reinterpret_cast<int32_t*>(p);
  p += gs_align_up((n > 0 ? n : 1) * 8, 256);
  if (n > 0 && hipMemsetAsync(*seg, 0, size_t(n) * 8, s) != hipSuccess) {
    gs_set_error("float64 grouping: memset failed");
    return GS_ERR_LAUNCH;
  }
  if (k == 0) return GS_OK;
  const int nb = int(gs_div_up(k, 256));
  hipLaunchKernelGGL(iota_kernel, dim3(nb), dim3(256), 0, s, k, iota);
  GS_CHECK_LAUNCH("float64 grouping/iota");
  if (int rc = gs_radix_sort_pairs(k, key_bytes, keys, iota, sorted_keys, *order, 0, 0, p,
                                   gs_sort_scratch_bytes(k, key_bytes), s))
    return rc;
  if (key_bytes == 4)
    hipLaunchKernelGGL(segments_kernel<uint32_t>, dim3(nb), dim3(256), 0, s, k,
                       static_cast<const uint32_t*>(sorted_keys), n, *seg);
  else
    hipLaunchKernelGGL(segments_kernel<uint64_t>, dim3(nb), dim3(256), 0, s, k,
                       static_cast<const uint64_t*>(sorted_keys), n, *seg);
  GS_CHECK_LAUNCH("float64 grouping/segments");
  return GS_OK;
}

extern "C" int64_t gs_raster_f64_scratch_bytes(int64_t v, int64_t k, int32_t num_features) {
  return records(k, num_features) + gs_f64_group_scratch_bytes(k, v, 4);
}

extern "C" int gs_raster_fwd_f64(int64_t v, int32_t num_features, const double* points, const double* features,
                                 const int32_t* tile_ranges, const int32_t* overlap_to_point, int64_t k,
                                 int32_t width, int32_t height, const GsRasterConfigF64* cfg, double* image,
                                 double* alpha, double* visibility, const double* background,
                                 int32_t background_offset, void* scratch, int64_t scratch_bytes, void* stream) {
  if (int rc = check_raster(v, num_features, points, features, tile_ranges, overlap_to_point, k, width, height, cfg,
                            image, alpha, scratch, scratch_bytes, "gs_raster_fwd_f64"))
    return rc;
  if (int rc = gs_check_background("gs_raster_fwd_f64", cfg->use_alpha_blending, background != nullptr,
                                   background_offset, num_features))
    return rc;
  const bool want_vis = cfg->compute_visibility != 0;
  GS_REQUIRE(!want_vis || v == 0 || visibility, GS_ERR_INVALID_ARGUMENT,
             "gs_raster_fwd_f64: NULL visibility with compute_visibility");
  hipStream_t s = static_cast<hipStream_t>(stream);
  TileArgs a = tile_args(v, num_features, points, features, tile_ranges, overlap_to_point, k, width, height, cfg, true);
  a.bg = background; a.bg_off = background ? background_offset : 0;
  const int tiles = a.tiles_x * int(gs_div_up(height, cfg->tile_size));
  double* rec = want_vis ? static_cast<double*>(scratch) : nullptr;
  if (rec && k > 0 && hipMemsetAsync(rec, 0, size_t(k) * 8, s) != hipSuccess) {  // entries in no tile's list
    gs_set_error("gs_raster_fwd_f64: memset failed");
    return GS_ERR_LAUNCH;
  }
  if (cfg->tile_size == 8) dispatch_fwd<8>(tiles, a, image, alpha, rec, s);
  else if (cfg->tile_size == 16) dispatch_fwd<16>(tiles, a, image, alpha, rec, s);
  else dispatch_fwd<32>(tiles, a, image, alpha, rec, s);
  GS_CHECK_LAUNCH("gs_raster_fwd_f64");
  if (!want_vis || v == 0) return GS_OK;
  int32_t *order, *seg;
  const int64_t rb = records(k, num_features);
  if (int rc = gs_f64_group(k, 4, overlap_to_point, v, &order, &seg, static_cast<char*>(scratch) + rb,
                            scratch_bytes - rb, s))
    return rc;
  hipLaunchKernelGGL(sum_records_kernel, dim3(gs_div_up(v, 256)), dim3(256), 0, s, v, 1, rec, order, seg, visibility,
                     1, nullptr, 0, nullptr);
  GS_CHECK_LAUNCH("gs_raster_fwd_f64/visibility");
  return GS_OK;
}

extern "C" int gs_raster_bwd_f64(int64_t v, int32_t num_features, const double* points, const double* features,
                                 const int32_t* tile_ranges, const int32_t* overlap_to_point, int64_t k,
                                 int32_t width, int32_t height, const GsRasterConfigF64* cfg, const double* image,
                                 const double* grad_image, const double* alpha, const double* grad_weight,
                                 double* grad_points, double* grad_features, double* point_heuristic, void* scratch,
                                 int64_t scratch_bytes, void* stream) {
  if (int rc = check_raster(v, num_features, points, features, tile_ranges, overlap_to_point, k, width, height, cfg,
                            image, grad_image, scratch, scratch_bytes, "gs_raster_bwd_f64"))
    return rc;
  GS_REQUIRE(cfg->use_alpha_blending, GS_ERR_UNSUPPORTED,
             "gs_raster_bwd_f64: use_alpha_blending = false has no backward (reference backward.py blends)");
  GS_REQUIRE(!grad_weight || alpha, GS_ERR_INVALID_ARGUMENT,
             "gs_raster_bwd_f64: grad_weight without the forward's alpha image");
  GS_REQUIRE(v == 0 || (grad_points && grad_features && (!cfg->compute_point_heuristic || point_heuristic)),
             GS_ERR_INVALID_ARGUMENT, "gs_raster_bwd_f64: NULL gradient buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  TileArgs a = tile_args(v, num_features, points, features, tile_ranges, overlap_to_point, k, width, height, cfg, false);
  a.alpha_in = alpha; a.grad_weight = grad_weight;
  const int tiles = a.tiles_x * int(gs_div_up(height, cfg->tile_size));
  const int R = 9 + num_features;
  double* rec = static_cast<double*>(scratch);
  if (k > 0 && hipMemsetAsync(rec, 0, size_t(k) * R * 8, s) != hipSuccess) {
    gs_set_error("gs_raster_bwd_f64: memset failed");
    return GS_ERR_LAUNCH;
  }
  if (cfg->tile_size == 8) dispatch_bwd<8>(tiles, a, image, grad_image, rec, s);
  else if (cfg->tile_size == 16) dispatch_bwd<16>(tiles, a, image, grad_image, rec, s);
  else dispatch_bwd<32>(tiles, a, image, grad_image, rec, s);
  GS_CHECK_LAUNCH("gs_raster_bwd_f64");
  if (v == 0) return GS_OK;
  int32_t *order, *seg;
  const int64_t rb = records(k, num_features);
  if (int rc = gs_f64_group(k, 4, overlap_to_point, v, &order, &seg, static_cast<char*>(scratch) + rb,
                            scratch_bytes - rb, s))
    return rc;
  hipLaunchKernelGGL(sum_records_kernel, dim3(gs_div_up(v, 256)), dim3(256), 0, s, v, R, rec, order, seg, grad_points,
                     7, grad_features, num_features, cfg->compute_point_heuristic ? point_heuristic : nullptr);
  GS_CHECK_LAUNCH("gs_raster_bwd_f64/sum");
  return GS_OK;
}
