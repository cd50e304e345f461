// depth_loss.hip -- depth-prior losses with a per-image scale / shift fit, forward and backward (gfx950), float and double.
//
// Per image b over pixels i with weight w_i (1 without a weight), x_i = depth_i or 1 / depth_i (inverse), p_i = prior_i:
//   a pixel is SELECTED OUT (adds nothing to any sum, gradient exactly 0) when w_i is not > 0, depth_i or prior_i is not
//   finite, or inverse and depth_i <= 0.
//   W = sum w, pm = sum w p / W, xm = sum w x / W, var_p = sum w (p - pm)^2, cov = sum w (p - pm)(x - xm), var_x likewise
//   kind 0 (L1):      align 0 (affine): s = cov / var_p, t = xm - s pm  (var_p <= 1e-12 sum w p^2: s = 0, t = xm)
//                     align 1 (scale):  s = sum w p x / sum w p^2, t = 0 (sum w p^2 = 0: s = 0)
//                     align 2 (none):   s = 1, t = 0
//                     r = x - s p - t,  L_b = sum w |r| / W,  loss = mean_b L_b
//   kind 1 (Pearson): rho = cov / sqrt(var_p var_x) (0 when W = 0, var_p <= 1e-12 sum w p^2 or var_x <= 1e-12 sum w x^2),
//                     loss = mean_b (1 - rho_b)
//   kind 2 (fit):     s and t of the align alone, no loss
// Everything between reading the inputs and rounding an output runs in double, for float inputs too: the operator is
// bound by its bytes, and in double the fit and the sign of every residual are those of the float inputs themselves.
//
// Launches.  Every image is cut into runs of DL_WAVE_ITEMS items (an item: one pixel, or 16 bytes of pixels where the
// pixel strides are 1 and rows and bases are 16-byte aligned), one wave per run, DL_WAVES runs per workgroup.
//   moments   a wave sums w, w dp, w dx, w dp^2, w dp dx, w dx^2 with dp = p - kp, dx = x - kx about a pivot (kp, kx) of
//             its own, its first selected pixel: no sum ever holds the square of an offset the data do not have.
//             8 doubles per wave go to scratch.
//   finish 0  one workgroup, image after image: W and the means from the waves' sums, then the centred and the raw
//             second moments with every wave's sums moved from its pivot to the mean; s, t (or rho) -> stats, results.
//   residual  a wave sums w |r|, w sgn(r) (p - pc), w sgn(r), w (pc = pm, or 0 for scale / none); 4 doubles per wave.
//   finish 1  L_b, the loss, and the backward's coefficients -> stats.
//   backward  one lane per item: d_depth = g_loss / B * w / W * (sgn(r) - c0 - c1 (p - pc)) [* -1 / depth^2].
// align none skips the moments, Pearson and fit the residual sweep.  Every sum has one program order given the shapes
// (lanes by butterfly, waves and runs in index order), no atomics: the outputs repeat bit for bit.  stats (B, 18)
// doubles stays on the device between the directions; nothing is read back.
#include <cmath>

#include "gs_common.h"

namespace {

constexpr int DL_THREADS = 256;
constexpr int DL_WAVES = DL_THREADS / GS_WAVE;
constexpr int DL_ITERS = 4;                          // items per lane, all loaded before the first is used
constexpr int DL_WAVE_ITEMS = GS_WAVE * DL_ITERS;    // 256
constexpr int DL_FINISH_THREADS = 512;
constexpr int DL_FINISH_WAVES = DL_FINISH_THREADS / GS_WAVE;
constexpr int DL_PART = 8;                           // doubles a wave leaves in scratch
constexpr int DL_STATS = 18;                         // doubles per image in stats
constexpr double DL_FLAT = 1e-12;
constexpr int64_t DL_MAX_BATCH = 65535;              // grid.y

enum { DL_L1 = 0, DL_PEARSON = 1, DL_FIT = 2 };
enum { DL_AFFINE = 0, DL_SCALE = 1, DL_NONE = 2 };
// stats row
enum { ST_W = 0, ST_PM, ST_XM, ST_VARP, ST_COV, ST_VARX, ST_SPP, ST_SPX, ST_SXX, ST_S, ST_T, ST_PC, ST_C0, ST_C1,
       ST_INVW, ST_VALUE, ST_PM_LO, ST_XM_LO };

template <typename T>
struct DlArgs {
  int batch, kind, align, inverse;
  unsigned items, per_row, nparts;  // per image
  int64_t pixels;                   // height * width
  int64_t width;
  const T* depth; int64_t dsb, dsr, dsp;
  const T* prior; int64_t psb, psr, psp;
  const T* weight; int64_t wsb, wsr, wsp;  // NULL: every weight 1
  double* partials;                 // (batch, nparts, DL_PART)
  double* stats;                    // (batch, DL_STATS)
  T* results;                       // 1 + 3 batch: loss, L_b (1 - rho_b), s_b (rho_b), t_b
  const T* g_loss;
  T* d_depth;                       // (batch, height, width) contiguous
};

template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) DlPack {
  T v[VEC];
};

template <typename T, int VEC>
struct DlRaw {
  DlPack<T, VEC> d, p, w;
};

// the item's pixels as stored; past the image: weight 0
template <typename T, int VEC>
__device__ __forceinline__ DlRaw<T, VEC> dl_load(const DlArgs<T>& a, int b, unsigned item) {
  DlRaw<T, VEC> r;
  if (item < a.items) {
    const unsigned row = item / a.per_row, col = (item - row * a.per_row) * VEC;
    r.d = *reinterpret_cast<const DlPack<T, VEC>*>(a.depth + b * a.dsb + row * a.dsr + col * a.dsp);
    r.p = *reinterpret_cast<const DlPack<T, VEC>*>(a.prior + b * a.psb + row * a.psr + col * a.psp);
    if (a.weight) {
      r.w = *reinterpret_cast<const DlPack<T, VEC>*>(a.weight + b * a.wsb + row * a.wsr + col * a.wsp);
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) r.w.v[e] = T(1);
    }
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) { r.d.v[e] = T(1); r.p.v[e] = T(0); r.w.v[e] = T(0); }
  }
  return r;
}

// the one place a pixel is selected: (w, p, x) in double, all 0 for a pixel that is selected out
template <typename T>
__device__ __forceinline__ void dl_pixel(T depth, T prior, T weight, int inverse, double& w, double& p, double& x) {
  const double d = double(depth), q = double(prior), ww = double(weight);
  const bool in = ww > 0.0 && fabs(d) < INFINITY && fabs(q) < INFINITY && (!inverse || d > 0.0);  // a NaN fails each
  const double xx = inverse ? 1.0 / (in ? d : 1.0) : d;
  w = in ? ww : 0.0;
  p = in ? q : 0.0;
  x = in ? xx : 0.0;
}

// forward and backward take the sign of the same expression
__device__ __forceinline__ double dl_residual(double x, double p, double s, double t) { return fma(-s, p, x) - t; }
__device__ __forceinline__ double dl_sign(double r) { return r > 0.0 ? 1.0 : (r < 0.0 ? -1.0 : 0.0); }

__device__ __forceinline__ double dl_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

template <typename T, int VEC>
__global__ __launch_bounds__(DL_THREADS) void depth_loss_moments_kernel(DlArgs<T> a) {
  const int b = blockIdx.y, lane = threadIdx.x & (GS_WAVE - 1);
  const unsigned run = blockIdx.x * DL_WAVES + (threadIdx.x >> 6);
  if (run >= a.nparts) return;  // the whole wave
  DlRaw<T, VEC> raw[DL_ITERS];
#pragma unroll
  for (int it = 0; it < DL_ITERS; ++it) raw[it] = dl_load<T, VEC>(a, b, run * DL_WAVE_ITEMS + it * GS_WAVE + lane);
  double kp = 0.0, kx = 0.0;
  bool pivot = false;  // the same in every lane
  double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int it = 0; it < DL_ITERS; ++it) {
    double w[VEC], p[VEC], x[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) dl_pixel(raw[it].d.v[e], raw[it].p.v[e], raw[it].w.v[e], a.inverse, w[e], p[e], x[e]);
    if (!pivot) {
      bool mine = false;
      double cp = 0.0, cx = 0.0;
#pragma unroll
      for (int e = VEC - 1; e >= 0; --e)
        if (w[e] > 0.0) { mine = true; cp = p[e]; cx = x[e]; }
      const unsigned long long any = __ballot(mine);
      if (any) {
        const int src = __ffsll(any) - 1;
        kp = __shfl(cp, src);
        kx = __shfl(cx, src);
        pivot = true;
      }
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double dp = p[e] - kp, dx = x[e] - kx, wp = w[e] * dp, wx = w[e] * dx;
      m[0] += w[e]; m[1] += wp; m[2] += wx;
      m[3] = fma(wp, dp, m[3]); m[4] = fma(wp, dx, m[4]); m[5] = fma(wx, dx, m[5]);
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) m[k] = dl_wave_sum(m[k]);
  if (lane == 0) {
    double* out = a.partials + (int64_t(b) * a.nparts + run) * DL_PART;
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = m[k];
    out[6] = kp;
    out[7] = kx;
  }
}

template <typename T, int VEC>
__global__ __launch_bounds__(DL_THREADS) void depth_loss_residual_kernel(DlArgs<T> a) {
  const int b = blockIdx.y, lane = threadIdx.x & (GS_WAVE - 1);
  const unsigned run = blockIdx.x * DL_WAVES + (threadIdx.x >> 6);
  if (run >= a.nparts) return;
  DlRaw<T, VEC> raw[DL_ITERS];
#pragma unroll
  for (int it = 0; it < DL_ITERS; ++it) raw[it] = dl_load<T, VEC>(a, b, run * DL_WAVE_ITEMS + it * GS_WAVE + lane);
  const double* st = a.stats + int64_t(b) * DL_STATS;
  const bool fitted = a.align != DL_NONE;
  const double s = fitted ? st[ST_S] : 1.0, t = fitted ? st[ST_T] : 0.0, pc = fitted ? st[ST_PC] : 0.0;
  double m[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int it = 0; it < DL_ITERS; ++it)
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      double w, p, x;
      dl_pixel(raw[it].d.v[e], raw[it].p.v[e], raw[it].w.v[e], a.inverse, w, p, x);
      const double r = dl_residual(x, p, s, t), ws = w * dl_sign(r);
      m[0] = fma(w, fabs(r), m[0]);
      m[1] = fma(ws, p - pc, m[1]);
      m[2] += ws;
      m[3] += w;
    }
#pragma unroll
  for (int k = 0; k < 4; ++k) m[k] = dl_wave_sum(m[k]);
  if (lane == 0) {
    double* out = a.partials + (int64_t(b) * a.nparts + run) * DL_PART;
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = m[k];
  }
}

// sums of N values over the workgroup, in every thread: lanes by butterfly, waves in index order
template <int N>
__device__ __forceinline__ void dl_block_sum(double (&v)[N], double (*s_red)[DL_PART]) {
  static_assert(N <= DL_PART, "s_red holds DL_PART sums a wave");
  const int lane = threadIdx.x & (GS_WAVE - 1), wave = threadIdx.x >> 6;
  __syncthreads();  // the round before has been read
#pragma unroll
  for (int k = 0; k < N; ++k) {
    v[k] = dl_wave_sum(v[k]);
    if (lane == 0) s_red[wave][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double sum = s_red[0][k];
#pragma unroll 1
    for (int w = 1; w < DL_FINISH_WAVES; ++w) sum += s_red[w][k];
    v[k] = sum;
  }
}

// STAGE 0: after the moments.  STAGE 1: after the residuals.  One workgroup, image after image.
template <typename T, int STAGE>
__global__ __launch_bounds__(DL_FINISH_THREADS) void depth_loss_finish_kernel(DlArgs<T> a) {
  __shared__ double s_red[DL_FINISH_WAVES][DL_PART];
  const double nan = __builtin_nan("");
  double loss = 0.0;
  for (int b = 0; b < a.batch; ++b) {
    const double* part = a.partials + int64_t(b) * a.nparts * DL_PART;
    double* st = a.stats + int64_t(b) * DL_STATS;
    T* res = a.results + 1 + b;  // L_b; s_b and t_b follow at + batch and + 2 batch
    if (STAGE == 0) {
      double f[3] = {0.0, 0.0, 0.0};
#pragma unroll 2
      for (unsigned j = threadIdx.x; j < a.nparts; j += DL_FINISH_THREADS) {
        const double* m = part + int64_t(j) * DL_PART;
        f[0] += m[0];
        f[1] += fma(m[0], m[6], m[1]);
        f[2] += fma(m[0], m[7], m[2]);
      }
      dl_block_sum<3>(f, s_red);
      const double W = f[0], pm = W > 0.0 ? f[1] / W : 0.0, xm = W > 0.0 ? f[2] / W : 0.0;
      // var_p, cov, var_x about the means; the raw sums of p^2, p x, x^2; what is left of sum w (p - pm), sum w (x - xm):
      // pm and xm are rounded to their own magnitude, the low parts carry them to the rounding of the spread
      double q[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
      for (unsigned j = threadIdx.x; j < a.nparts; j += DL_FINISH_THREADS) {
        const double* m = part + int64_t(j) * DL_PART;
        const double kp = m[6], kx = m[7], ep = pm - kp, ex = xm - kx;
        q[0] += m[3] - 2.0 * ep * m[1] + m[0] * ep * ep;
        q[1] += m[4] - ep * m[2] - ex * m[1] + m[0] * ep * ex;
        q[2] += m[5] - 2.0 * ex * m[2] + m[0] * ex * ex;
        q[3] += m[3] + 2.0 * kp * m[1] + m[0] * kp * kp;
        q[4] += m[4] + kp * m[2] + kx * m[1] + m[0] * kp * kx;
        q[5] += m[5] + 2.0 * kx * m[2] + m[0] * kx * kx;
        q[6] += m[1] - ep * m[0];
        q[7] += m[2] - ex * m[0];
      }
      dl_block_sum<8>(q, s_red);
      if (threadIdx.x != 0) continue;
      const double varp = fmax(q[0], 0.0), cov = q[1], varx = fmax(q[2], 0.0), spp = q[3], spx = q[4], sxx = q[5];
      st[ST_W] = W; st[ST_PM] = pm; st[ST_XM] = xm; st[ST_VARP] = varp; st[ST_COV] = cov; st[ST_VARX] = varx;
      st[ST_SPP] = spp; st[ST_SPX] = spx; st[ST_SXX] = sxx;
      st[ST_INVW] = W > 0.0 ? 1.0 / W : 0.0;
      st[ST_PM_LO] = W > 0.0 ? q[6] / W : 0.0;
      st[ST_XM_LO] = W > 0.0 ? q[7] / W : 0.0;
      const bool flat_p = !(varp > DL_FLAT * spp);
      if (a.kind == DL_PEARSON) {
        const bool flat = !(W > 0.0) || flat_p || !(varx > DL_FLAT * sxx);
        const double root = flat ? 1.0 : sqrt(varp * varx), rho = flat ? 0.0 : cov / root;
        st[ST_C0] = flat ? 0.0 : 1.0 / root;
        st[ST_C1] = flat ? 0.0 : rho / varx;
        st[ST_VALUE] = rho;
        res[0] = T(1.0 - rho);
        res[a.batch] = T(rho);
        res[2 * a.batch] = T(0);
        loss += 1.0 - rho;
      } else {
        double s = 1.0, t = 0.0, pc = 0.0;
        if (a.align == DL_AFFINE) {
          s = flat_p ? 0.0 : cov / varp;
          t = xm - s * pm;
          pc = pm;
        } else if (a.align == DL_SCALE) {
          s = spp > 0.0 ? spx / spp : 0.0;
        }
        st[ST_S] = s; st[ST_T] = t; st[ST_PC] = pc;
        if (a.kind == DL_FIT) {
          res[0] = T(nan);
          res[a.batch] = T(W > 0.0 ? s : nan);
          res[2 * a.batch] = T(W > 0.0 ? t : nan);
        }
      }
    } else {
      double f[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
      for (unsigned j = threadIdx.x; j < a.nparts; j += DL_FINISH_THREADS) {
        const double* m = part + int64_t(j) * DL_PART;
#pragma unroll
        for (int k = 0; k < 4; ++k) f[k] += m[k];
      }
      dl_block_sum<4>(f, s_red);
      if (threadIdx.x != 0) continue;
      const double W = f[3], inv = W > 0.0 ? 1.0 / W : 0.0, L = W > 0.0 ? f[0] / W : 0.0;
      double s = 1.0, t = 0.0, c0 = 0.0, c1 = 0.0;
      if (a.align == DL_NONE) {
        st[ST_W] = W; st[ST_S] = 1.0; st[ST_T] = 0.0; st[ST_PC] = 0.0;
      } else {
        s = st[ST_S]; t = st[ST_T];
        if (a.align == DL_AFFINE) {
          c0 = f[2] * inv;
          c1 = st[ST_VARP] > DL_FLAT * st[ST_SPP] ? f[1] / st[ST_VARP] : 0.0;
        } else {
          c1 = st[ST_SPP] > 0.0 ? f[1] / st[ST_SPP] : 0.0;
        }
      }
      st[ST_C0] = c0; st[ST_C1] = c1; st[ST_INVW] = inv; st[ST_VALUE] = L;
      res[0] = T(W > 0.0 ? L : nan);
      res[a.batch] = T(W > 0.0 ? s : nan);
      res[2 * a.batch] = T(W > 0.0 ? t : nan);
      loss += L;
    }
  }
  if (threadIdx.x == 0 && (STAGE == 1 || a.kind != DL_L1))
    a.results[0] = a.kind == DL_FIT ? T(0) : T(loss / double(a.batch));
}

template <typename T, int VEC>
__global__ __launch_bounds__(DL_THREADS) void depth_loss_bwd_kernel(DlArgs<T> a) {
  const int b = blockIdx.y;
  const unsigned item = blockIdx.x * DL_THREADS + threadIdx.x;
  if (item >= a.items) return;
  const DlRaw<T, VEC> raw = dl_load<T, VEC>(a, b, item);
  const double* st = a.stats + int64_t(b) * DL_STATS;
  const double up = double(*a.g_loss) / double(a.batch);
  const double s = st[ST_S], t = st[ST_T], pc = st[ST_PC], c0 = st[ST_C0], c1 = st[ST_C1], inv = st[ST_INVW];
  const double pm = st[ST_PM], xm = st[ST_XM], pm_lo = st[ST_PM_LO], xm_lo = st[ST_XM_LO];
  DlPack<T, VEC> out;
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    double w, p, x;
    dl_pixel(raw.d.v[e], raw.p.v[e], raw.w.v[e], a.inverse, w, p, x);
    double g;
    if (a.kind == DL_PEARSON) g = -(up * w) * (c0 * ((p - pm) - pm_lo) - c1 * ((x - xm) - xm_lo));
    else g = (up * w * inv) * (dl_sign(dl_residual(x, p, s, t)) - c0 - c1 * (p - pc));
    if (a.inverse) g *= -(x * x);  // dx / d depth = -1 / depth^2
    out.v[e] = w > 0.0 ? T(g) : T(0);
  }
  const unsigned row = item / a.per_row, col = (item - row * a.per_row) * VEC;
  *reinterpret_cast<DlPack<T, VEC>*>(a.d_depth + int64_t(b) * a.pixels + int64_t(row) * a.width + col) = out;
}

// ------------------------------------------------------------------------------------------------------------- host
int dl_sizes(const char* who, int64_t batch, int64_t height, int64_t width) {
  GS_REQUIRE(batch >= 1 && height >= 1 && width >= 1, GS_ERR_INVALID_ARGUMENT, "%s: images %lld x %lld x %lld are empty",
             who, (long long)batch, (long long)height, (long long)width);
  const int64_t top = int64_t(1) << 31;
  GS_REQUIRE(batch < top && height < top && width < top && height * width < top && batch * height * width < top,
             GS_ERR_UNSUPPORTED, "%s: images %lld x %lld x %lld above 2^31 pixels", who, (long long)batch,
             (long long)height, (long long)width);
  GS_REQUIRE(batch <= DL_MAX_BATCH, GS_ERR_UNSUPPORTED, "%s: batch %lld above %lld", who, (long long)batch,
             (long long)DL_MAX_BATCH);
  return GS_OK;
}

int64_t dl_parts(int64_t items) { return gs_div_up(items, DL_WAVE_ITEMS); }

int dl_strides(const char* who, const char* name, int64_t batch, int64_t height, int64_t width, int64_t sb, int64_t sr,
               int64_t sp, bool shared) {
  GS_REQUIRE(sp >= 1 && sr >= width * sp && (batch == 1 || (shared && sb == 0) || sb >= height * sr),
             GS_ERR_INVALID_ARGUMENT,
             "%s: bad strides of %s (batch %lld, row %lld, pixel %lld elements for %lld x %lld x %lld)", who, name,
             (long long)sb, (long long)sr, (long long)sp, (long long)batch, (long long)height, (long long)width);
  return GS_OK;
}

template <typename T>
bool dl_wide(const T* ptr, int64_t sb, int64_t sr, int64_t sp, int64_t width) {
  constexpr int64_t VEC = 16 / sizeof(T);
  return sp == 1 && width % VEC == 0 && sr % VEC == 0 && sb % VEC == 0 && reinterpret_cast<uintptr_t>(ptr) % 16 == 0;
}

// what both directions check and fill alike; *wide: 16-byte items
template <typename T>
int dl_common(const char* who, int64_t batch, int64_t height, int64_t width, const T* depth, int64_t dsb, int64_t dsr,
              int64_t dsp, const T* prior, int64_t psb, int64_t psr, int64_t psp, const T* weight, int64_t wsb,
              int64_t wsr, int64_t wsp, int32_t kind, int32_t align, int32_t inverse, const void* out,
              const void* stats, DlArgs<T>* a, bool* wide) {
  GS_TRY(dl_sizes(who, batch, height, width));
  GS_REQUIRE(depth != nullptr && prior != nullptr && out != nullptr && stats != nullptr, GS_ERR_INVALID_ARGUMENT,
             "%s: NULL buffer (depth / prior / output / stats)", who);
  GS_TRY(dl_strides(who, "depth", batch, height, width, dsb, dsr, dsp, false));
  GS_TRY(dl_strides(who, "prior", batch, height, width, psb, psr, psp, false));
  if (weight) GS_TRY(dl_strides(who, "weight", batch, height, width, wsb, wsr, wsp, true));
  GS_REQUIRE(kind >= DL_L1 && kind <= DL_FIT && align >= DL_AFFINE && align <= DL_NONE && (inverse == 0 || inverse == 1),
             GS_ERR_UNSUPPORTED, "%s: unknown mode (kind %d, align %d, inverse %d)", who, kind, align, inverse);
  *wide = dl_wide(depth, dsb, dsr, dsp, width) && dl_wide(prior, psb, psr, psp, width) &&
          (!weight || dl_wide(weight, wsb, wsr, wsp, width));
  a->batch = int(batch); a->kind = kind; a->align = align; a->inverse = inverse;
  a->pixels = height * width; a->width = width;
  a->depth = depth; a->dsb = dsb; a->dsr = dsr; a->dsp = dsp;
  a->prior = prior; a->psb = psb; a->psr = psr; a->psp = psp;
  a->weight = weight; a->wsb = wsb; a->wsr = wsr; a->wsp = wsp;
  a->partials = nullptr; a->stats = nullptr; a->results = nullptr; a->g_loss = nullptr; a->d_depth = nullptr;
  return GS_OK;
}

template <typename T>
void dl_set_items(DlArgs<T>* a, int64_t height, int64_t width, bool wide) {
  const int64_t vec = wide ? int64_t(16 / sizeof(T)) : 1;
  a->per_row = unsigned(width / vec);
  a->items = unsigned(height * (width / vec));
  a->nparts = unsigned(dl_parts(a->items));
}

template <typename T>
int dl_fwd(const char* who, int64_t batch, int64_t height, int64_t width, const T* depth, int64_t dsb, int64_t dsr,
           int64_t dsp, const T* prior, int64_t psb, int64_t psr, int64_t psp, const T* weight, int64_t wsb,
           int64_t wsr, int64_t wsp, int32_t kind, int32_t align, int32_t inverse, T* results, double* stats,
           void* scratch, int64_t scratch_bytes, void* stream) {
  DlArgs<T> a;
  bool wide = false;
  GS_TRY(dl_common(who, batch, height, width, depth, dsb, dsr, dsp, prior, psb, psr, psp, weight, wsb, wsr, wsp, kind,
                   align, inverse, results, stats, &a, &wide));
  GS_TRY(gs_check_scratch(who, scratch, scratch_bytes, batch * dl_parts(height * width) * DL_PART * 8));
  constexpr int VEC = 16 / sizeof(T);
  dl_set_items(&a, height, width, wide);
  a.partials = static_cast<double*>(scratch); a.stats = stats; a.results = results;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(unsigned(gs_div_up(a.nparts, DL_WAVES)), unsigned(batch)), block(DL_THREADS);
  if (!(kind == DL_L1 && align == DL_NONE)) {
    if (wide) hipLaunchKernelGGL((depth_loss_moments_kernel<T, VEC>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((depth_loss_moments_kernel<T, 1>), grid, block, 0, st, a);
    GS_CHECK_LAUNCH(who);
    hipLaunchKernelGGL((depth_loss_finish_kernel<T, 0>), dim3(1), dim3(DL_FINISH_THREADS), 0, st, a);
    GS_CHECK_LAUNCH(who);
  }
  if (kind == DL_L1) {
    if (wide) hipLaunchKernelGGL((depth_loss_residual_kernel<T, VEC>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((depth_loss_residual_kernel<T, 1>), grid, block, 0, st, a);
    GS_CHECK_LAUNCH(who);
    hipLaunchKernelGGL((depth_loss_finish_kernel<T, 1>), dim3(1), dim3(DL_FINISH_THREADS), 0, st, a);
    GS_CHECK_LAUNCH(who);
  }
  return GS_OK;
}

template <typename T>
int dl_bwd(const char* who, int64_t batch, int64_t height, int64_t width, const T* depth, int64_t dsb, int64_t dsr,
           int64_t dsp, const T* prior, int64_t psb, int64_t psr, int64_t psp, const T* weight, int64_t wsb,
           int64_t wsr, int64_t wsp, int32_t kind, int32_t align, int32_t inverse, const double* stats, const T* g_loss,
           T* d_depth, void* stream) {
  DlArgs<T> a;
  bool wide = false;
  GS_TRY(dl_common(who, batch, height, width, depth, dsb, dsr, dsp, prior, psb, psr, psp, weight, wsb, wsr, wsp, kind,
                   align, inverse, d_depth, stats, &a, &wide));
  GS_REQUIRE(g_loss != nullptr, GS_ERR_INVALID_ARGUMENT, "%s: NULL buffer (g_loss)", who);
  GS_REQUIRE(kind != DL_FIT, GS_ERR_UNSUPPORTED, "%s: unknown mode (kind %d has no backward)", who, kind);
  constexpr int VEC = 16 / sizeof(T);
  wide = wide && reinterpret_cast<uintptr_t>(d_depth) % 16 == 0;
  dl_set_items(&a, height, width, wide);
  a.stats = const_cast<double*>(stats); a.g_loss = g_loss; a.d_depth = d_depth;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(unsigned(gs_div_up(a.items, DL_THREADS)), unsigned(batch)), block(DL_THREADS);
  if (wide) hipLaunchKernelGGL((depth_loss_bwd_kernel<T, VEC>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((depth_loss_bwd_kernel<T, 1>), grid, block, 0, st, a);
  GS_CHECK_LAUNCH(who);
  return GS_OK;
}

}  // namespace

extern "C" int64_t gs_depth_loss_scratch_bytes(int64_t batch, int64_t height, int64_t width) {
  GS_TRY(dl_sizes("gs_depth_loss_scratch_bytes", batch, height, width));
  return batch * dl_parts(height * width) * DL_PART * 8;
}

#define DL_STRIDED(T, name) const T* name, int64_t name##_batch_stride, int64_t name##_row_stride, int64_t name##_pixel_stride
#define DL_PASS(name) name, name##_batch_stride, name##_row_stride, name##_pixel_stride

extern "C" int gs_depth_loss_fwd(int64_t batch, int64_t height, int64_t width, DL_STRIDED(float, depth),
                                 DL_STRIDED(float, prior), DL_STRIDED(float, weight), int32_t kind, int32_t align,
                                 int32_t inverse, float* results, double* stats, void* scratch, int64_t scratch_bytes,
                                 void* stream) {
  return dl_fwd<float>("gs_depth_loss_fwd", batch, height, width, DL_PASS(depth), DL_PASS(prior), DL_PASS(weight), kind,
                       align, inverse, results, stats, scratch, scratch_bytes, stream);
}

extern "C" int gs_depth_loss_fwd_f64(int64_t batch, int64_t height, int64_t width, DL_STRIDED(double, depth),
                                     DL_STRIDED(double, prior), DL_STRIDED(double, weight), int32_t kind, int32_t align,
                                     int32_t inverse, double* results, double* stats, void* scratch,
                                     int64_t scratch_bytes, void* stream) {
  return dl_fwd<double>("gs_depth_loss_fwd_f64", batch, height, width, DL_PASS(depth), DL_PASS(prior), DL_PASS(weight),
                        kind, align, inverse, results, stats, scratch, scratch_bytes, stream);
}

extern "C" int gs_depth_loss_bwd(int64_t batch, int64_t height, int64_t width, DL_STRIDED(float, depth),
                                 DL_STRIDED(float, prior), DL_STRIDED(float, weight), int32_t kind, int32_t align,
                                 int32_t inverse, const double* stats, const float* g_loss, float* d_depth,
                                 void* stream) {
  return dl_bwd<float>("gs_depth_loss_bwd", batch, height, width, DL_PASS(depth), DL_PASS(prior), DL_PASS(weight), kind,
                       align, inverse, stats, g_loss, d_depth, stream);
}

extern "C" int gs_depth_loss_bwd_f64(int64_t batch, int64_t height, int64_t width, DL_STRIDED(double, depth),
                                     DL_STRIDED(double, prior), DL_STRIDED(double, weight), int32_t kind, int32_t align,
                                     int32_t inverse, const double* stats, const double* g_loss, double* d_depth,
                                     void* stream) {
  return dl_bwd<double>("gs_depth_loss_bwd_f64", batch, height, width, DL_PASS(depth), DL_PASS(prior), DL_PASS(weight),
                        kind, align, inverse, stats, g_loss, d_depth, stream);
}
