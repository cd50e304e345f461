// loss.hip -- fused photometric loss (1 - l) * mean|x - y| + l * (1 - SSIM(x, y)), forward and backward, on
// channel-last images (H, W, C) / (B, H, W, C) as the rasterizer writes them (include/gsplat_hip.h, "photometric
// loss").  SSIM with a separable Gaussian window g (x) g, zero padding:
//   mu_x = g*x, var_x = g*x^2 - mu_x^2, cov = g*xy - mu_x mu_y,
//   m = (2 mu_x mu_y + C1)(2 cov + C2) / ((mu_x^2 + mu_y^2 + C1)(var_x + var_y + C2)).
//
// One workgroup of 256 lanes owns a 16 x 16 pixel tile and up to LOSS_CB channels.  It loads the (16 + ws - 1)^2 halo
// of both images into LDS (planar per channel, so the horizontal taps are one element apart), runs the horizontal pass
// of the five moments into a second LDS buffer and the vertical pass per output pixel in registers.
//
// Shifted moments: float32 loses var = E[x^2] - mu^2 to cancellation exactly where training converges (smooth, flat or
// nearly equal images).  Variance and covariance do not change when a constant is subtracted, so every tile works on
// shifted values, with pivots taken at the tile's centre pixel (clamped into the image).  Zero padding remains zero
// padding of the UNSHIFTED image: a padded tap holds minus the pivot.
//
// Difference form: the second image enters as d = x - y, not as y.  The five moments are those of xs = x - c and
// ds = d - k (pivots c = x(centre), k = d(centre)), and with mu_d = mu_x - mu_y, var_d = var(x - y), cov_xd:
//   b1 = mu_x^2 + mu_y^2 + C1,  b2 = var_x + var_y + C2 = 2 (var_x - cov_xd) + var_d + C2,
//   2 mu_x mu_y + C1 = b1 - mu_d^2,  2 cov_xy + C2 = b2 - var_d,
//   m = (1 - p)(1 - q),  p = mu_d^2 / b1,  q = var_d / b2.
// 1 - m is built from the small quantities themselves, so the map keeps its relative accuracy as the render approaches
// the target (and ssim(x, x) is exactly 1).  With S2 = (sum of the rounded weights)^2 and e = 1 - S2 (a few ulp, formed
// on the host in double), the separable sums of the shifted values give
//   e_x = g*xs - c e = mu_x - c,  var_x = g*xs^2 - e_x^2 + c^2 e,  cov_xd = g*xs ds - e_x e_d + c k e,  likewise e_d, var_d.
//
// Backward, with L = dm/dmu_x (second moments fixed), B = dm/dvar_x, Cq = dm/dcov_xy at pixel q and u the upstream
// gradient of m(q):  d_x(p) = sum_q w(q - p) u(q) [L + 2 (x(p) - mu_x(q)) B + (y(p) - mu_y(q)) Cq]
//                           = sum_q w(q - p) u(q) [L + D (x(p) - mu_x(q)) - Cq (d(p) - mu_d(q))],  D = 2 B + Cq.
// B and Cq are each ~1/C2 and nearly cancel; D = Cq q and L = 2 (1 - q)(mu_x p - mu_d) / b1 are formed without that
// cancellation.  Folding mu_x, mu_d into the first map would make it large and let it cancel against x g*(uD) and
// d g*(uC) later, so the forward saves A' = L - D e_x + Cq e_d (relative to the pivots of q's tile), D and Cq; the
// backward tile with pivots c_p, k_p re-bases halo pixels of neighbouring tiles,
//   A'' = A' + (c_p - c_q) D - (k_p - k_q) Cq,
//   d_x(p) = g*(u A'') + (x(p) - c_p) g*(u D) - (d(p) - k_p) g*(u Cq)  (+ the L1 term),
// written straight into d_image: three saved maps, no large terms.
//
// The scalars are deterministic: every workgroup writes its two partial sums (double) to scratch and one small
// launch adds them in a fixed order.  No float atomics anywhere.
//
// Per-pixel weights (the gs_photo_loss_weighted_* entry points): w(b, p) >= 0, one per pixel, shared by the channels,
// weights both means and leaves the map alone:  L = sum w |x - y| / (C S),  M = sum_counted w m / (C S_v),  S = sum w,
// S_v = sum of w over the counted pixels.  The forward multiplies w(p) into its two sums at the output pixel; the
// workgroups of channel group 0 also write sum w and sum counted w of their tile, and the finish launch divides by
// C S and C S_v.  The backward multiplies the mean's upstream by w(q) at the halo pixel q and the L1 term by w(p), and
// reads S, S_v from device memory as the forward left them.  A term whose weight sum is zero gives 0 to the loss and
// to the gradient, and NaN as its part.  WT = false compiles the unweighted kernels as they were.

#include <cmath>

#include "gs_common.h"

namespace {

constexpr int LOSS_T = 16;       // tile edge in pixels; one lane per pixel
constexpr int LOSS_MIN_CB = 2;
// channels per workgroup: 4, or 2 in float64 (the generic-window halo of four double channels would not fit the 64 KiB
// of static LDS)
template <typename T>
constexpr int loss_cb() { return sizeof(T) == 8 ? LOSS_MIN_CB : 4; }
constexpr int LOSS_MAX_WS = 15;

template <typename T>
struct LossImage {
  const T* p;
  int64_t sb, sr, sp;  // batch / row / pixel stride in elements; channels contiguous
};

template <typename T>
struct LossWeight {
  const T* p;          // one weight per pixel
  int64_t sb, sr, sp;  // batch (0 = the same weights for every batch entry) / row / pixel stride in elements
};

template <typename T>
struct LossWindow {
  T w[LOSS_MAX_WS];
  T d;  // 1 - (sum of w)^2, formed in double
  int ws;
};

template <typename T>
struct LossFwdArgs {
  LossImage<T> x, y;
  int batch, height, width, channels, chunks;
  LossWindow<T> win;
  T c1, c2;
  int valid, do_ssim;
  T* map;       // (B,H,W,C) or null
  T* saved;     // 3 x (B,H,W,C): A', D, C; or null
  int64_t plane;  // B*H*W*C
  double* partials;  // 2 per workgroup: sum |x - y|, sum of the (masked) ssim map
  LossWeight<T> w;    // the weighted kernels only
  double* wpartials;  // 2 per pixel tile and batch entry: sum w, sum of the counted w
};

template <typename T>
struct LossBwdArgs {
  LossImage<T> x, y;
  int batch, height, width, channels, chunks;
  LossWindow<T> win;
  int valid;
  const T* saved;
  int64_t plane;
  const T* upstream;  // (B,H,W,C) gradient of the map, or null
  const T* grad;      // device scalar multiplying both coefficients, or null (= 1)
  T l1_coeff, ssim_coeff;  // already divided by the element counts
  T* d_image;         // (B,H,W,C) contiguous
  LossWeight<T> w;    // the weighted kernels only, which divide the raw coefficients by C S and C S_v themselves
  const T* norm;      // device [S, S_v] as the weighted forward wrote them
  double l1_raw, ssim_raw;
};

template <typename T>
__device__ __forceinline__ T loss_abs(T v) { return v < T(0) ? -v : v; }

// lane t < ws copies weight t into LDS with constant indices into the by-value argument (a dynamic index would send
// the array through scratch)
template <typename T>
__device__ __forceinline__ void loss_stage_window(const LossWindow<T>& win, T* s_w, int tid) {
  T v = T(0);
#pragma unroll
  for (int k = 0; k < LOSS_MAX_WS; ++k)
    if (tid == k) v = win.w[k];
  if (tid < LOSS_MAX_WS) s_w[tid] = v;
}

__device__ __forceinline__ double loss_block_sum(double v, double* s_red, int tid) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  if ((tid & 63) == 0) s_red[tid >> 6] = v;
  __syncthreads();
  const double total = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
  __syncthreads();
  return total;
}

template <typename T>
__device__ __forceinline__ T loss_weight_at(const LossWeight<T>& w, int b, int gy, int gx) {
  return w.p[int64_t(b) * w.sb + gy * w.sr + gx * w.sp];
}

// the tile's sum w and sum of the counted w; channel group 0 alone, as the weights have no channel axis
template <typename T>
__device__ __forceinline__ void loss_weight_partials(const LossFwdArgs<T>& a, int b, T w_all, T w_counted,
                                                     double* s_red, int tid) {
  const double total = loss_block_sum(double(w_all), s_red, tid);
  const double counted = loss_block_sum(double(w_counted), s_red, tid);
  if (tid == 0) {
    const int64_t tile = (int64_t(b) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    a.wpartials[2 * tile] = total;
    a.wpartials[2 * tile + 1] = counted;
  }
}

// the weighted backward's coefficients: l1_raw / (C S) and ssim_raw / (C S_v) formed in double as the host forms
// l1_coeff / count, and 0 for a term without weight
template <typename T>
__device__ __forceinline__ void loss_weighted_coeffs(const LossBwdArgs<T>& a, T* l1, T* ss) {
  const double S = double(a.norm[0]), Sv = double(a.norm[1]);
  *l1 = S > 0.0 ? T(a.l1_raw / (double(a.channels) * S)) : T(0);
  *ss = Sv > 0.0 ? T(a.ssim_raw / (double(a.channels) * Sv)) : T(0);
}

// WS: the window size the loops are unrolled for, or 0 = any odd size up to LOSS_MAX_WS (weights read from LDS)
// WT: per-pixel weights (a.w)
template <typename T, int WS, bool WT>
__global__ __launch_bounds__(256) void photo_loss_fwd_kernel(LossFwdArgs<T> a) {
  constexpr int LOSS_CB = loss_cb<T>();
  constexpr int RMAX = WS ? WS / 2 : LOSS_MAX_WS / 2;
  constexpr int HALO = LOSS_T + 2 * RMAX, PLANE = HALO * HALO;
  static_assert(2 * PLANE >= 4 * LOSS_T * LOSS_T, "a channel's dead halo planes stage its four outputs");
  __shared__ T s_halo[LOSS_CB * 2 * PLANE];  // [channel][x | x - y][row][pixel], shifted by the pivots
  __shared__ T s_h[5 * HALO * LOSS_T];       // horizontal sums [moment][row][column]
  __shared__ T s_w[16];
  __shared__ T s_piv[2 * LOSS_CB];           // [channel][c | k]
  __shared__ double s_red[4];

  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int ws = WS ? WS : a.win.ws, R = ws >> 1, halo = LOSS_T + 2 * R;
  const int b = blockIdx.z / a.chunks, c0 = (blockIdx.z % a.chunks) * LOSS_CB;
  const int nc = min(LOSS_CB, a.channels - c0);
  const int x0 = blockIdx.x * LOSS_T, y0 = blockIdx.y * LOSS_T;
  const int H = a.height, W = a.width;
  const T* xb = a.x.p + int64_t(b) * a.x.sb + c0;
  const T* yb = a.y.p + int64_t(b) * a.y.sb + c0;

  loss_stage_window(a.win, s_w, tid);
  if (tid < 2 * nc) {
    const int ch = tid >> 1, cy = min(y0 + LOSS_T / 2, H - 1), cx = min(x0 + LOSS_T / 2, W - 1);
    const T xc = xb[cy * a.x.sr + cx * a.x.sp + ch];
    s_piv[tid] = (tid & 1) ? xc - yb[cy * a.y.sr + cx * a.y.sp + ch] : xc;
  }
  __syncthreads();

  for (int i = tid; i < halo * halo * nc; i += 256) {
    const int ch = i % nc, p = i / nc, px = p % halo, row = p / halo;
    const int gy = y0 - R + row, gx = x0 - R + px;
    T xv = T(0), yv = T(0);
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      xv = xb[gy * a.x.sr + gx * a.x.sp + ch];
      yv = yb[gy * a.y.sr + gx * a.y.sp + ch];
    }
    T* dst = s_halo + ch * 2 * PLANE + row * HALO + px;
    dst[0] = xv - s_piv[2 * ch];
    dst[PLANE] = (xv - yv) - s_piv[2 * ch + 1];
  }
  __syncthreads();

  T g[WS ? WS : 1];
  if (WS) {
#pragma unroll
    for (int k = 0; k < (WS ? WS : 1); ++k) g[k] = s_w[k];
  }

  const int gy = y0 + ty, gx = x0 + tx;
  const bool inside = gy < H && gx < W;
  const bool counted = inside && (!a.valid || (gy >= R && gy < H - R && gx >= R && gx < W - R));
  T l1_sum = T(0), ssim_sum = T(0);
  T wp = T(0);
  if (WT && inside) wp = loss_weight_at(a.w, b, gy, gx);

  for (int ch = 0; ch < nc; ++ch) {
    const T* hx = s_halo + ch * 2 * PLANE;
    const T* hd = hx + PLANE;
    for (int i = tid; i < halo * LOSS_T; i += 256) {
      const int row = i >> 4, col = i & 15;
      const T* rx = hx + row * HALO + col;
      const T* rd = hd + row * HALO + col;
      T sx = T(0), sd = T(0), sxx = T(0), sdd = T(0), sxd = T(0);
#pragma unroll
      for (int k = 0; k < ws; ++k) {
        const T wk = WS ? g[WS ? k : 0] : s_w[k];
        const T xv = rx[k], dv = rd[k], wx = wk * xv, wd = wk * dv;
        sx += wx; sd += wd; sxx += wx * xv; sdd += wd * dv; sxd += wx * dv;
      }
      s_h[i] = sx; s_h[HALO * LOSS_T + i] = sd; s_h[2 * HALO * LOSS_T + i] = sxx;
      s_h[3 * HALO * LOSS_T + i] = sdd; s_h[4 * HALO * LOSS_T + i] = sxd;
    }
    __syncthreads();
    T ex = T(0), ed = T(0), vxx = T(0), vdd = T(0), vxd = T(0);
#pragma unroll
    for (int k = 0; k < ws; ++k) {
      const T wk = WS ? g[WS ? k : 0] : s_w[k];
      const int at = (ty + k) * LOSS_T + tx;
      ex += wk * s_h[at]; ed += wk * s_h[HALO * LOSS_T + at]; vxx += wk * s_h[2 * HALO * LOSS_T + at];
      vdd += wk * s_h[3 * HALO * LOSS_T + at]; vxd += wk * s_h[4 * HALO * LOSS_T + at];
    }
    __syncthreads();  // s_h and this channel's halo planes are dead from here

    const T cx = s_piv[2 * ch], ck = s_piv[2 * ch + 1], e = a.win.d;
    ex -= cx * e; ed -= ck * e;
    const T mux = ex + cx, mud = ed + ck, muy = mux - mud;
    const T varx = (vxx - ex * ex) + cx * cx * e, vard = (vdd - ed * ed) + ck * ck * e;
    const T covxd = (vxd - ex * ed) + cx * ck * e;
    const T b1 = mux * mux + muy * muy + a.c1, b2 = T(2) * (varx - covxd) + vard + a.c2;
    const T p = mud * mud / b1, q = vard / b2;
    const T P = T(1) - p, Q = T(1) - q, m = P * Q;
    if (counted) ssim_sum += WT ? wp * m : m;
    if (inside) {
      const T xv = xb[gy * a.x.sr + gx * a.x.sp + ch], yv = yb[gy * a.y.sr + gx * a.y.sp + ch];
      l1_sum += WT ? wp * loss_abs(xv - yv) : loss_abs(xv - yv);
    }
    T* stage = s_halo + ch * 2 * PLANE;
    stage[tid] = m;
    if (a.saved) {
      const T L = T(2) * Q * (mux * p - mud) / b1;
      const T Cq = T(2) * P / b2, Dq = Cq * q;
      stage[256 + tid] = L - Dq * ex + Cq * ed;
      stage[512 + tid] = Dq;
      stage[768 + tid] = Cq;
    }
  }
  __syncthreads();

  if (a.map || a.saved) {
    for (int i = tid; i < 256 * nc; i += 256) {
      const int ch = i % nc, p = i / nc, oy = y0 + (p >> 4), ox = x0 + (p & 15);
      if (oy >= H || ox >= W) continue;
      const int64_t at = ((int64_t(b) * H + oy) * W + ox) * a.channels + c0 + ch;
      const T* stage = s_halo + ch * 2 * PLANE + p;
      if (a.map) a.map[at] = stage[0];
      if (a.saved) {
        a.saved[at] = stage[256];
        a.saved[a.plane + at] = stage[512];
        a.saved[2 * a.plane + at] = stage[768];
      }
    }
  }

  const double l1_total = loss_block_sum(double(l1_sum), s_red, tid);
  const double ssim_total = loss_block_sum(double(ssim_sum), s_red, tid);
  if (tid == 0) {
    const int64_t wg = (int64_t(blockIdx.z) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    a.partials[2 * wg] = l1_total;
    a.partials[2 * wg + 1] = ssim_total;
  }
  if (WT && c0 == 0) loss_weight_partials(a, b, wp, counted ? wp : T(0), s_red, tid);
}

// ssim_weight = 0: the same grid and partials, nothing but |x - y|
template <typename T, bool WT>
__global__ __launch_bounds__(256) void photo_loss_l1_fwd_kernel(LossFwdArgs<T> a) {
  constexpr int LOSS_CB = loss_cb<T>();
  __shared__ double s_red[4];
  const int tid = threadIdx.x;
  const int b = blockIdx.z / a.chunks, c0 = (blockIdx.z % a.chunks) * LOSS_CB;
  const int nc = min(LOSS_CB, a.channels - c0);
  const int x0 = blockIdx.x * LOSS_T, y0 = blockIdx.y * LOSS_T;
  const T* xb = a.x.p + int64_t(b) * a.x.sb + c0;
  const T* yb = a.y.p + int64_t(b) * a.y.sb + c0;
  T l1_sum = T(0);
  for (int i = tid; i < 256 * nc; i += 256) {
    const int ch = i % nc, p = i / nc, gy = y0 + (p / LOSS_T), gx = x0 + (p % LOSS_T);
    if (gy < a.height && gx < a.width) {
      const T v = loss_abs(xb[gy * a.x.sr + gx * a.x.sp + ch] - yb[gy * a.y.sr + gx * a.y.sp + ch]);
      l1_sum += WT ? loss_weight_at(a.w, b, gy, gx) * v : v;
    }
  }
  const double total = loss_block_sum(double(l1_sum), s_red, tid);
  if (tid == 0) {
    const int64_t wg = (int64_t(blockIdx.z) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    a.partials[2 * wg] = total;
    a.partials[2 * wg + 1] = 0.0;
  }
  if (WT && c0 == 0) {
    const int gy = y0 + tid / LOSS_T, gx = x0 + tid % LOSS_T, R = a.win.ws >> 1;
    const bool inside = gy < a.height && gx < a.width;
    const bool counted = inside && (!a.valid || (gy >= R && gy < a.height - R && gx >= R && gx < a.width - R));
    const T wp = inside ? loss_weight_at(a.w, b, gy, gx) : T(0);
    loss_weight_partials(a, b, wp, counted ? wp : T(0), s_red, tid);
  }
}

// one workgroup: the partials in a fixed order, in double; results = [loss, l1_mean, ssim_mean], and with nres == 5 also
// [S, S_v].  wpartials (nw pairs) or null: the weight sums that replace the host's counts, count = channels * sum.  A
// weighted term with no weight adds nothing to the loss and reports NaN.
template <typename T>
__global__ __launch_bounds__(256) void photo_loss_finish_kernel(const double* partials, int64_t n, double count_l1,
                                                               double count_ssim, double ssim_weight, int do_ssim,
                                                               const double* wpartials, int64_t nw, double channels,
                                                               int nres, T* results) {
  __shared__ double s_l1[256], s_ss[256];
  const int tid = threadIdx.x;
  double l1 = 0.0, ss = 0.0;
  for (int64_t i = tid; i < n; i += 256) { l1 += partials[2 * i]; ss += partials[2 * i + 1]; }
  s_l1[tid] = l1; s_ss[tid] = ss;
  __syncthreads();
  for (int half = 128; half >= 1; half >>= 1) {
    if (tid < half) { s_l1[tid] += s_l1[tid + half]; s_ss[tid] += s_ss[tid + half]; }
    __syncthreads();
  }
  const double l1_total = s_l1[0], ss_total = s_ss[0];
  double S = count_l1 / channels, Sv = count_ssim / channels;
  if (wpartials) {
    __syncthreads();
    double w = 0.0, wv = 0.0;
    for (int64_t i = tid; i < nw; i += 256) { w += wpartials[2 * i]; wv += wpartials[2 * i + 1]; }
    s_l1[tid] = w; s_ss[tid] = wv;
    __syncthreads();
    for (int half = 128; half >= 1; half >>= 1) {
      if (tid < half) { s_l1[tid] += s_l1[tid + half]; s_ss[tid] += s_ss[tid + half]; }
      __syncthreads();
    }
    S = s_l1[0]; Sv = s_ss[0];
    count_l1 = channels * S; count_ssim = channels * Sv;
  }
  if (tid == 0) {
    const bool has_l1 = !wpartials || S > 0.0, has_ssim = do_ssim && (!wpartials || Sv > 0.0);
    const double l1_mean = has_l1 ? l1_total / count_l1 : nan("");
    const double ssim_mean = has_ssim ? ss_total / count_ssim : nan("");
    double loss = 0.0;
    if (has_l1 && has_ssim) loss = (1.0 - ssim_weight) * l1_mean + ssim_weight * (1.0 - ssim_mean);
    else if (has_l1) loss = (1.0 - ssim_weight) * l1_mean;
    else if (has_ssim) loss = ssim_weight * (1.0 - ssim_mean);
    results[0] = T(loss);
    results[1] = T(l1_mean);
    results[2] = T(ssim_mean);
    if (nres == 5) { results[3] = T(S); results[4] = T(Sv); }
  }
}

template <typename T, int WS, bool WT>
__global__ __launch_bounds__(256) void photo_loss_bwd_kernel(LossBwdArgs<T> a) {
  constexpr int LOSS_CB = loss_cb<T>();
  constexpr int RMAX = WS ? WS / 2 : LOSS_MAX_WS / 2;
  constexpr int HALO = LOSS_T + 2 * RMAX, PLANE = HALO * HALO;
  __shared__ T s_halo[LOSS_CB * 3 * PLANE];  // [channel][u A'' | u D | u C][row][pixel]
  __shared__ T s_h[3 * HALO * LOSS_T];
  __shared__ T s_w[16];
  __shared__ T s_piv[9 * 2 * LOSS_CB];       // [neighbour tile 3 x 3][channel][c | k]

  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int ws = WS ? WS : a.win.ws, R = ws >> 1, halo = LOSS_T + 2 * R;
  const int b = blockIdx.z / a.chunks, c0 = (blockIdx.z % a.chunks) * LOSS_CB;
  const int nc = min(LOSS_CB, a.channels - c0);
  const int x0 = blockIdx.x * LOSS_T, y0 = blockIdx.y * LOSS_T;
  const int H = a.height, W = a.width;
  const T* xb = a.x.p + int64_t(b) * a.x.sb + c0;
  const T* yb = a.y.p + int64_t(b) * a.y.sb + c0;
  const T gl = a.grad ? a.grad[0] : T(1);
  T l1_coeff = a.l1_coeff, ssim_coeff = a.ssim_coeff;
  if (WT) loss_weighted_coeffs(a, &l1_coeff, &ssim_coeff);
  const T u_mean = ssim_coeff * gl;

  loss_stage_window(a.win, s_w, tid);
  if (tid < 18 * nc) {
    // the forward pivots of the 3 x 3 tiles around this one (tiles off the image are never referred to)
    const int t = tid / (2 * nc), r = tid % (2 * nc), ch = r >> 1;
    const int ny = min(max(int(blockIdx.y) + t / 3 - 1, 0), int(gridDim.y) - 1);
    const int nx = min(max(int(blockIdx.x) + t % 3 - 1, 0), int(gridDim.x) - 1);
    const int cy = min(ny * LOSS_T + LOSS_T / 2, H - 1), cx = min(nx * LOSS_T + LOSS_T / 2, W - 1);
    const T xc = xb[cy * a.x.sr + cx * a.x.sp + ch];
    s_piv[(t * LOSS_CB + ch) * 2 + (r & 1)] = (r & 1) ? xc - yb[cy * a.y.sr + cx * a.y.sp + ch] : xc;
  }
  __syncthreads();

  for (int i = tid; i < halo * halo * nc; i += 256) {
    const int ch = i % nc, p = i / nc, px = p % halo, row = p / halo;
    const int gy = y0 - R + row, gx = x0 - R + px;
    T ua = T(0), ub = T(0), uc = T(0);
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const int64_t at = ((int64_t(b) * H + gy) * W + gx) * a.channels + c0 + ch;
      T u = T(0);
      // one weight per halo pixel: the lanes of its channels read the same address
      if (!a.valid || (gy >= R && gy < H - R && gx >= R && gx < W - R))
        u = WT ? u_mean * loss_weight_at(a.w, b, gy, gx) : u_mean;
      if (a.upstream) u += a.upstream[at];
      const T A = a.saved[at], Dq = a.saved[a.plane + at], Cq = a.saved[2 * a.plane + at];
      const int t = ((gy >> 4) - int(blockIdx.y) + 1) * 3 + ((gx >> 4) - int(blockIdx.x) + 1);
      const T* pq = s_piv + (t * LOSS_CB + ch) * 2;
      const T* pp = s_piv + (4 * LOSS_CB + ch) * 2;
      const T App = A + (pp[0] - pq[0]) * Dq - (pp[1] - pq[1]) * Cq;
      ua = u * App; ub = u * Dq; uc = u * Cq;
    }
    T* dst = s_halo + ch * 3 * PLANE + row * HALO + px;
    dst[0] = ua; dst[PLANE] = ub; dst[2 * PLANE] = uc;
  }
  __syncthreads();

  T g[WS ? WS : 1];
  if (WS) {
#pragma unroll
    for (int k = 0; k < (WS ? WS : 1); ++k) g[k] = s_w[k];
  }

  const int gy = y0 + ty, gx = x0 + tx;
  const bool inside = gy < H && gx < W;
  T u_l1 = l1_coeff * gl;
  if (WT && inside) u_l1 *= loss_weight_at(a.w, b, gy, gx);

  for (int ch = 0; ch < nc; ++ch) {
    const T* ha = s_halo + ch * 3 * PLANE;
    for (int i = tid; i < halo * LOSS_T; i += 256) {
      const int row = i >> 4, col = i & 15;
      const T* r = ha + row * HALO + col;
      T sa = T(0), sb = T(0), sc = T(0);
#pragma unroll
      for (int k = 0; k < ws; ++k) {
        const T wk = WS ? g[WS ? k : 0] : s_w[k];
        sa += wk * r[k]; sb += wk * r[PLANE + k]; sc += wk * r[2 * PLANE + k];
      }
      s_h[i] = sa; s_h[HALO * LOSS_T + i] = sb; s_h[2 * HALO * LOSS_T + i] = sc;
    }
    __syncthreads();
    T ga = T(0), gb = T(0), gc = T(0);
#pragma unroll
    for (int k = 0; k < ws; ++k) {
      const T wk = WS ? g[WS ? k : 0] : s_w[k];
      const int at = (ty + k) * LOSS_T + tx;
      ga += wk * s_h[at]; gb += wk * s_h[HALO * LOSS_T + at]; gc += wk * s_h[2 * HALO * LOSS_T + at];
    }
    __syncthreads();
    T dx = T(0);
    if (inside) {
      const T xv = xb[gy * a.x.sr + gx * a.x.sp + ch], yv = yb[gy * a.y.sr + gx * a.y.sp + ch];
      const T* pp = s_piv + (4 * LOSS_CB + ch) * 2;
      const T diff = xv - yv;
      dx = ga + (xv - pp[0]) * gb - (diff - pp[1]) * gc;
      dx += diff > T(0) ? u_l1 : (diff < T(0) ? -u_l1 : T(0));
    }
    s_halo[ch * 3 * PLANE + tid] = dx;
  }
  __syncthreads();

  for (int i = tid; i < 256 * nc; i += 256) {
    const int ch = i % nc, p = i / nc, oy = y0 + (p >> 4), ox = x0 + (p & 15);
    if (oy >= H || ox >= W) continue;
    a.d_image[((int64_t(b) * H + oy) * W + ox) * a.channels + c0 + ch] = s_halo[ch * 3 * PLANE + p];
  }
}

// no SSIM term: d_image = coefficient * sign(x - y)
template <typename T, bool WT>
__global__ __launch_bounds__(256) void photo_loss_l1_bwd_kernel(LossBwdArgs<T> a) {
  constexpr int LOSS_CB = loss_cb<T>();
  const int tid = threadIdx.x;
  const int b = blockIdx.z / a.chunks, c0 = (blockIdx.z % a.chunks) * LOSS_CB;
  const int nc = min(LOSS_CB, a.channels - c0);
  const int x0 = blockIdx.x * LOSS_T, y0 = blockIdx.y * LOSS_T;
  const T* xb = a.x.p + int64_t(b) * a.x.sb + c0;
  const T* yb = a.y.p + int64_t(b) * a.y.sb + c0;
  T l1_coeff = a.l1_coeff, ssim_coeff = a.ssim_coeff;
  if (WT) loss_weighted_coeffs(a, &l1_coeff, &ssim_coeff);
  const T u_tile = l1_coeff * (a.grad ? a.grad[0] : T(1));
  for (int i = tid; i < 256 * nc; i += 256) {
    const int ch = i % nc, p = i / nc, gy = y0 + (p / LOSS_T), gx = x0 + (p % LOSS_T);
    if (gy >= a.height || gx >= a.width) continue;
    const T u_l1 = WT ? u_tile * loss_weight_at(a.w, b, gy, gx) : u_tile;
    const T diff = xb[gy * a.x.sr + gx * a.x.sp + ch] - yb[gy * a.y.sr + gx * a.y.sp + ch];
    a.d_image[((int64_t(b) * a.height + gy) * a.width + gx) * a.channels + c0 + ch] =
        diff > T(0) ? u_l1 : (diff < T(0) ? -u_l1 : T(0));
  }
}

// ---------------------------------------------------------------------------------------------------- host side
int loss_window(int ws, double sigma, double* out) {
  GS_REQUIRE(ws >= 3 && ws <= LOSS_MAX_WS && (ws & 1), GS_ERR_INVALID_ARGUMENT,
             "window_size %d: an odd size from 3 to %d", ws, LOSS_MAX_WS);
  GS_REQUIRE(sigma > 0.0 && std::isfinite(sigma), GS_ERR_INVALID_ARGUMENT, "sigma %g must be positive", sigma);
  double sum = 0.0;
  for (int i = 0; i < ws; ++i) {
    const double t = double(i) - 0.5 * double(ws - 1);
    out[i] = exp(-(t * t) / (2.0 * sigma * sigma));
    sum += out[i];
  }
  for (int i = 0; i < ws; ++i) out[i] /= sum;
  return GS_OK;
}

template <typename T>
int loss_make_window(int ws, double sigma, LossWindow<T>* win) {
  double w[LOSS_MAX_WS];
  const int rc = loss_window(ws, sigma, w);
  if (rc != GS_OK) return rc;
  double sum = 0.0;
  for (int i = 0; i < LOSS_MAX_WS; ++i) {
    win->w[i] = i < ws ? T(w[i]) : T(0);
    sum += double(win->w[i]);
  }
  win->d = T(1.0 - sum * sum);
  win->ws = ws;
  return GS_OK;
}

struct LossShape {
  int64_t batch, height, width, channels;
  int64_t chunks, tiles_x, tiles_y, groups;
};

int loss_shape(const char* who, int cb, int64_t batch, int64_t height, int64_t width, int64_t channels, LossShape* s) {
  GS_REQUIRE(batch >= 0 && height >= 0 && width >= 0, GS_ERR_INVALID_ARGUMENT, "%s: negative size", who);
  GS_REQUIRE(channels >= 1, GS_ERR_INVALID_ARGUMENT, "%s: channels %lld", who, (long long)channels);
  GS_REQUIRE(height < (1 << 20) && width < (1 << 20) && channels < (1 << 20), GS_ERR_UNSUPPORTED,
             "%s: image %lld x %lld x %lld too large", who, (long long)height, (long long)width, (long long)channels);
  s->batch = batch; s->height = height; s->width = width; s->channels = channels;
  s->chunks = gs_div_up(channels, cb);
  s->tiles_x = gs_div_up(width, LOSS_T);
  s->tiles_y = gs_div_up(height, LOSS_T);
  s->groups = batch * s->chunks * s->tiles_x * s->tiles_y;
  GS_REQUIRE(batch * s->chunks <= 65535 && s->tiles_y <= 65535, GS_ERR_UNSUPPORTED,
             "%s: batch x channel groups %lld or tile rows %lld above the grid limit", who,
             (long long)(batch * s->chunks), (long long)s->tiles_y);
  return GS_OK;
}

template <typename T>
int loss_image(const char* who, const char* name, const LossShape& s, const T* p, int64_t sb, int64_t sr, int64_t sp,
               LossImage<T>* out) {
  GS_REQUIRE(p != nullptr, GS_ERR_INVALID_ARGUMENT, "%s: NULL buffer (%s)", who, name);
  GS_REQUIRE(sp >= s.channels && sr >= s.width * sp && (s.batch <= 1 || sb >= s.height * sr), GS_ERR_INVALID_ARGUMENT,
             "%s: bad strides of %s (batch %lld, row %lld, pixel %lld elements for %lld x %lld x %lld)", who, name,
             (long long)sb, (long long)sr, (long long)sp, (long long)s.height, (long long)s.width,
             (long long)s.channels);
  out->p = p; out->sb = sb; out->sr = sr; out->sp = sp;
  return GS_OK;
}

// what a weighted entry point adds to the unweighted argument list; weight == NULL runs unweighted
template <typename T>
struct LossWeighted {
  const T* weight;
  int64_t sb, sr, sp;
  const T* norm;  // backward: device [S, S_v]
};

template <typename T>
int loss_weight(const char* who, const LossShape& s, const LossWeighted<T>& wt, LossWeight<T>* out) {
  GS_REQUIRE(wt.sp >= 1 && wt.sr >= s.width * wt.sp && (wt.sb == 0 || wt.sb >= s.height * wt.sr),
             GS_ERR_INVALID_ARGUMENT,
             "%s: bad strides of weight (batch %lld, row %lld, pixel %lld elements for %lld x %lld; batch 0 = broadcast)",
             who, (long long)wt.sb, (long long)wt.sr, (long long)wt.sp, (long long)s.height, (long long)s.width);
  out->p = wt.weight; out->sb = wt.sb; out->sr = wt.sr; out->sp = wt.sp;
  return GS_OK;
}

int64_t loss_tiles(int64_t batch, int64_t height, int64_t width) {
  return batch * gs_div_up(width, LOSS_T) * gs_div_up(height, LOSS_T);
}

#define LOSS_TRY(expr)          \
  do {                          \
    const int rc_ = (expr);     \
    if (rc_ != GS_OK) return rc_; \
  } while (0)

template <typename T>
int loss_fwd(const char* who, int64_t batch, int64_t height, int64_t width, int64_t channels, const T* image,
             int64_t isb, int64_t isr, int64_t isp, const T* target, int64_t tsb, int64_t tsr, int64_t tsp,
             int32_t ws, double sigma, double data_range, double ssim_weight, int32_t valid, T* ssim_map,
             T* saved_maps, void* scratch, int64_t scratch_bytes, T* results, void* stream,
             const LossWeighted<T>* wt = nullptr) {
  LossShape s;
  LossFwdArgs<T> a;
  LOSS_TRY(loss_shape(who, loss_cb<T>(), batch, height, width, channels, &s));
  LOSS_TRY(loss_make_window(ws, sigma, &a.win));
  GS_REQUIRE(data_range > 0.0 && std::isfinite(data_range), GS_ERR_INVALID_ARGUMENT, "%s: data_range %g", who, data_range);
  GS_REQUIRE(ssim_weight >= 0.0 && ssim_weight <= 1.0, GS_ERR_INVALID_ARGUMENT, "%s: ssim_weight %g outside [0, 1]",
             who, ssim_weight);
  if (s.groups == 0) return GS_OK;
  GS_REQUIRE(!valid || (height >= ws && width >= ws), GS_ERR_INVALID_ARGUMENT,
             "%s: valid padding needs an image of at least %d x %d, got %lld x %lld", who, ws, ws, (long long)height,
             (long long)width);
  LOSS_TRY(loss_image(who, "image", s, image, isb, isr, isp, &a.x));
  LOSS_TRY(loss_image(who, "target", s, target, tsb, tsr, tsp, &a.y));
  const bool weighted = wt && wt->weight;
  a.w = LossWeight<T>{nullptr, 0, 0, 0};
  if (weighted) LOSS_TRY(loss_weight(who, s, *wt, &a.w));
  GS_REQUIRE(results != nullptr && scratch != nullptr, GS_ERR_INVALID_ARGUMENT, "%s: NULL buffer (results / scratch)",
             who);
  GS_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 8 == 0, GS_ERR_INVALID_ARGUMENT,
             "%s: scratch must be 8-byte aligned", who);
  const int64_t unweighted_need = gs_photo_loss_scratch_bytes(batch, height, width, channels);  // one size for both dtypes
  const int64_t need = wt ? gs_photo_loss_weighted_scratch_bytes(batch, height, width, channels) : unweighted_need;
  GS_REQUIRE(scratch_bytes >= need, GS_ERR_SCRATCH_TOO_SMALL, "%s: scratch %lld < %lld bytes", who,
             (long long)scratch_bytes, (long long)need);
  a.batch = int(batch); a.height = int(height); a.width = int(width); a.channels = int(channels);
  a.chunks = int(s.chunks);
  a.c1 = T((0.01 * data_range) * (0.01 * data_range));
  a.c2 = T((0.03 * data_range) * (0.03 * data_range));
  a.valid = valid ? 1 : 0;
  a.do_ssim = (ssim_weight != 0.0 || ssim_map || saved_maps) ? 1 : 0;
  a.map = ssim_map; a.saved = saved_maps;
  a.plane = batch * height * width * channels;
  a.partials = static_cast<double*>(scratch);
  a.wpartials = weighted ? reinterpret_cast<double*>(static_cast<char*>(scratch) + unweighted_need) : nullptr;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(unsigned(s.tiles_x), unsigned(s.tiles_y), unsigned(batch * s.chunks));
  if (weighted) {
    if (!a.do_ssim) hipLaunchKernelGGL((photo_loss_l1_fwd_kernel<T, true>), grid, dim3(256), 0, st, a);
    else if (ws == 11) hipLaunchKernelGGL((photo_loss_fwd_kernel<T, 11, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((photo_loss_fwd_kernel<T, 0, true>), grid, dim3(256), 0, st, a);
  } else {
    if (!a.do_ssim) hipLaunchKernelGGL((photo_loss_l1_fwd_kernel<T, false>), grid, dim3(256), 0, st, a);
    else if (ws == 11) hipLaunchKernelGGL((photo_loss_fwd_kernel<T, 11, false>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((photo_loss_fwd_kernel<T, 0, false>), grid, dim3(256), 0, st, a);
  }
  GS_CHECK_LAUNCH(who);
  const double count = double(a.plane);
  const double count_ssim =
      valid ? double(batch) * double(height - ws + 1) * double(width - ws + 1) * double(channels) : count;
  hipLaunchKernelGGL(photo_loss_finish_kernel<T>, dim3(1), dim3(256), 0, st, a.partials, s.groups, count, count_ssim,
                     ssim_weight, a.do_ssim, a.wpartials, loss_tiles(batch, height, width), double(channels),
                     wt ? 5 : 3, results);
  GS_CHECK_LAUNCH(who);
  return GS_OK;
}

template <typename T>
int loss_bwd(const char* who, int64_t batch, int64_t height, int64_t width, int64_t channels, const T* image,
             int64_t isb, int64_t isr, int64_t isp, const T* target, int64_t tsb, int64_t tsr, int64_t tsp,
             int32_t ws, double sigma, int32_t valid, const T* saved_maps, const T* upstream_map, const T* grad_loss,
             double l1_coeff, double ssim_coeff, T* d_image, void* stream, const LossWeighted<T>* wt = nullptr) {
  LossShape s;
  LossBwdArgs<T> a;
  LOSS_TRY(loss_shape(who, loss_cb<T>(), batch, height, width, channels, &s));
  LOSS_TRY(loss_make_window(ws, sigma, &a.win));
  GS_REQUIRE(std::isfinite(l1_coeff) && std::isfinite(ssim_coeff), GS_ERR_INVALID_ARGUMENT, "%s: coefficients %g, %g", who,
             l1_coeff, ssim_coeff);
  if (s.groups == 0) return GS_OK;
  GS_REQUIRE(!valid || (height >= ws && width >= ws), GS_ERR_INVALID_ARGUMENT,
             "%s: valid padding needs an image of at least %d x %d, got %lld x %lld", who, ws, ws, (long long)height,
             (long long)width);
  LOSS_TRY(loss_image(who, "image", s, image, isb, isr, isp, &a.x));
  LOSS_TRY(loss_image(who, "target", s, target, tsb, tsr, tsp, &a.y));
  const bool weighted = wt && wt->weight;
  a.w = LossWeight<T>{nullptr, 0, 0, 0};
  if (weighted) LOSS_TRY(loss_weight(who, s, *wt, &a.w));
  const bool do_ssim = ssim_coeff != 0.0 || upstream_map != nullptr;
  GS_REQUIRE(d_image != nullptr && (!do_ssim || saved_maps != nullptr), GS_ERR_INVALID_ARGUMENT,
             "%s: NULL buffer (d_image / saved_maps)", who);
  GS_REQUIRE(!wt || wt->norm != nullptr, GS_ERR_INVALID_ARGUMENT, "%s: NULL buffer (normalisers)", who);
  a.norm = wt ? wt->norm : nullptr;
  a.l1_raw = l1_coeff; a.ssim_raw = ssim_coeff;
  a.batch = int(batch); a.height = int(height); a.width = int(width); a.channels = int(channels);
  a.chunks = int(s.chunks);
  a.valid = valid ? 1 : 0;
  a.saved = saved_maps; a.upstream = upstream_map; a.grad = grad_loss;
  a.plane = batch * height * width * channels;
  const double count = double(a.plane);
  const double count_ssim =
      valid ? double(batch) * double(height - ws + 1) * double(width - ws + 1) * double(channels) : count;
  a.l1_coeff = T(l1_coeff / count);
  a.ssim_coeff = T(ssim_coeff / count_ssim);
  a.d_image = d_image;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(unsigned(s.tiles_x), unsigned(s.tiles_y), unsigned(batch * s.chunks));
  if (weighted) {
    if (!do_ssim) hipLaunchKernelGGL((photo_loss_l1_bwd_kernel<T, true>), grid, dim3(256), 0, st, a);
    else if (ws == 11) hipLaunchKernelGGL((photo_loss_bwd_kernel<T, 11, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((photo_loss_bwd_kernel<T, 0, true>), grid, dim3(256), 0, st, a);
  } else {
    if (!do_ssim) hipLaunchKernelGGL((photo_loss_l1_bwd_kernel<T, false>), grid, dim3(256), 0, st, a);
    else if (ws == 11) hipLaunchKernelGGL((photo_loss_bwd_kernel<T, 11, false>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((photo_loss_bwd_kernel<T, 0, false>), grid, dim3(256), 0, st, a);
  }
  GS_CHECK_LAUNCH(who);
  return GS_OK;
}

}  // namespace

extern "C" int gs_ssim_window(int32_t window_size, double sigma, float* host_out) {
  double w[LOSS_MAX_WS];
  const int rc = loss_window(window_size, sigma, w);
  if (rc != GS_OK) return rc;
  GS_REQUIRE(host_out != nullptr, GS_ERR_INVALID_ARGUMENT, "gs_ssim_window: NULL host_out");
  for (int i = 0; i < window_size; ++i) host_out[i] = float(w[i]);
  return GS_OK;
}

extern "C" int64_t gs_photo_loss_scratch_bytes(int64_t batch, int64_t height, int64_t width, int64_t channels) {
  if (batch < 0 || height < 0 || width < 0 || channels < 1) return 0;
  return batch * gs_div_up(channels, LOSS_MIN_CB) * gs_div_up(width, LOSS_T) * gs_div_up(height, LOSS_T) * 16;
}

extern "C" int gs_photo_loss_fwd(int64_t batch, int64_t height, int64_t width, int64_t channels, const float* image,
                                 int64_t image_batch_stride, int64_t image_row_stride, int64_t image_pixel_stride,
                                 const float* target, int64_t target_batch_stride, int64_t target_row_stride,
                                 int64_t target_pixel_stride, int32_t window_size, double sigma, double data_range,
                                 double ssim_weight, int32_t valid, float* ssim_map, float* saved_maps, void* scratch,
                                 int64_t scratch_bytes, float* results, void* stream) {
  return loss_fwd<float>("gs_photo_loss_fwd", batch, height, width, channels, image, image_batch_stride,
                         image_row_stride, image_pixel_stride, target, target_batch_stride, target_row_stride,
                         target_pixel_stride, window_size, sigma, data_range, ssim_weight, valid, ssim_map, saved_maps,
                         scratch, scratch_bytes, results, stream);
}

extern "C" int gs_photo_loss_fwd_f64(int64_t batch, int64_t height, int64_t width, int64_t channels,
                                     const double* image, int64_t image_batch_stride, int64_t image_row_stride,
                                     int64_t image_pixel_stride, const double* target, int64_t target_batch_stride,
                                     int64_t target_row_stride, int64_t target_pixel_stride, int32_t window_size,
                                     double sigma, double data_range, double ssim_weight, int32_t valid,
                                     double* ssim_map, double* saved_maps, void* scratch, int64_t scratch_bytes,
                                     double* results, void* stream) {
  return loss_fwd<double>("gs_photo_loss_fwd_f64", batch, height, width, channels, image, image_batch_stride,
                          image_row_stride, image_pixel_stride, target, target_batch_stride, target_row_stride,
                          target_pixel_stride, window_size, sigma, data_range, ssim_weight, valid, ssim_map,
                          saved_maps, scratch, scratch_bytes, results, stream);
}

extern "C" int gs_photo_loss_bwd(int64_t batch, int64_t height, int64_t width, int64_t channels, const float* image,
                                 int64_t image_batch_stride, int64_t image_row_stride, int64_t image_pixel_stride,
                                 const float* target, int64_t target_batch_stride, int64_t target_row_stride,
                                 int64_t target_pixel_stride, int32_t window_size, double sigma, int32_t valid,
                                 const float* saved_maps, const float* upstream_map, const float* grad_loss,
                                 double l1_coeff, double ssim_coeff, float* d_image, void* stream) {
  return loss_bwd<float>("gs_photo_loss_bwd", batch, height, width, channels, image, image_batch_stride,
                         image_row_stride, image_pixel_stride, target, target_batch_stride, target_row_stride,
                         target_pixel_stride, window_size, sigma, valid, saved_maps, upstream_map, grad_loss, l1_coeff,
                         ssim_coeff, d_image, stream);
}

extern "C" int gs_photo_loss_bwd_f64(int64_t batch, int64_t height, int64_t width, int64_t channels,
                                     const double* image, int64_t image_batch_stride, int64_t image_row_stride,
                                     int64_t image_pixel_stride, const double* target, int64_t target_batch_stride,
                                     int64_t target_row_stride, int64_t target_pixel_stride, int32_t window_size,
                                     double sigma, int32_t valid, const double* saved_maps,
                                     const double* upstream_map, const double* grad_loss, double l1_coeff,
                                     double ssim_coeff, double* d_image, void* stream) {
  return loss_bwd<double>("gs_photo_loss_bwd_f64", batch, height, width, channels, image, image_batch_stride,
                          image_row_stride, image_pixel_stride, target, target_batch_stride, target_row_stride,
                          target_pixel_stride, window_size, sigma, valid, saved_maps, upstream_map, grad_loss,
                          l1_coeff, ssim_coeff, d_image, stream);
}

extern "C" int64_t gs_photo_loss_weighted_scratch_bytes(int64_t batch, int64_t height, int64_t width,
                                                        int64_t channels) {
  if (batch < 0 || height < 0 || width < 0 || channels < 1) return 0;
  return gs_photo_loss_scratch_bytes(batch, height, width, channels) + loss_tiles(batch, height, width) * 16;
}

extern "C" int gs_photo_loss_weighted_fwd(int64_t batch, int64_t height, int64_t width, int64_t channels,
                                          const float* image, int64_t image_batch_stride, int64_t image_row_stride,
                                          int64_t image_pixel_stride, const float* target, int64_t target_batch_stride,
                                          int64_t target_row_stride, int64_t target_pixel_stride,
                                          const float* weight, int64_t weight_batch_stride, int64_t weight_row_stride,
                                          int64_t weight_pixel_stride, int32_t window_size, double sigma,
                                          double data_range, double ssim_weight, int32_t valid, float* ssim_map,
                                          float* saved_maps, void* scratch, int64_t scratch_bytes, float* results,
                                          void* stream) {
  const LossWeighted<float> wt{weight, weight_batch_stride, weight_row_stride, weight_pixel_stride, nullptr};
  return loss_fwd<float>("gs_photo_loss_weighted_fwd", batch, height, width, channels, image, image_batch_stride,
                         image_row_stride, image_pixel_stride, target, target_batch_stride, target_row_stride,
                         target_pixel_stride, window_size, sigma, data_range, ssim_weight, valid, ssim_map, saved_maps,
                         scratch, scratch_bytes, results, stream, &wt);
}

extern "C" int gs_photo_loss_weighted_fwd_f64(int64_t batch, int64_t height, int64_t width, int64_t channels,
                                              const double* image, int64_t image_batch_stride,
                                              int64_t image_row_stride, int64_t image_pixel_stride,
                                              const double* target, int64_t target_batch_stride,
                                              int64_t target_row_stride, int64_t target_pixel_stride,
                                              const double* weight, int64_t weight_batch_stride,
                                              int64_t weight_row_stride, int64_t weight_pixel_stride,
                                              int32_t window_size, double sigma, double data_range, double ssim_weight,
                                              int32_t valid, double* ssim_map, double* saved_maps, void* scratch,
                                              int64_t scratch_bytes, double* results, void* stream) {
  const LossWeighted<double> wt{weight, weight_batch_stride, weight_row_stride, weight_pixel_stride, nullptr};
  return loss_fwd<double>("gs_photo_loss_weighted_fwd_f64", batch, height, width, channels, image, image_batch_stride,
                          image_row_stride, image_pixel_stride, target, target_batch_stride, target_row_stride,
                          target_pixel_stride, window_size, sigma, data_range, ssim_weight, valid, ssim_map,
                          saved_maps, scratch, scratch_bytes, results, stream, &wt);
}

extern "C" int gs_photo_loss_weighted_bwd(int64_t batch, int64_t height, int64_t width, int64_t channels,
                                          const float* image, int64_t image_batch_stride, int64_t image_row_stride,
                                          int64_t image_pixel_stride, const float* target, int64_t target_batch_stride,
                                          int64_t target_row_stride, int64_t target_pixel_stride,
                                          const float* weight, int64_t weight_batch_stride, int64_t weight_row_stride,
                                          int64_t weight_pixel_stride, const float* normalisers, int32_t window_size,
                                          double sigma, int32_t valid, const float* saved_maps,
                                          const float* upstream_map, const float* grad_loss, double l1_coeff,
                                          double ssim_coeff, float* d_image, void* stream) {
  const LossWeighted<float> wt{weight, weight_batch_stride, weight_row_stride, weight_pixel_stride, normalisers};
  return loss_bwd<float>("gs_photo_loss_weighted_bwd", batch, height, width, channels, image, image_batch_stride,
                         image_row_stride, image_pixel_stride, target, target_batch_stride, target_row_stride,
                         target_pixel_stride, window_size, sigma, valid, saved_maps, upstream_map, grad_loss, l1_coeff,
                         ssim_coeff, d_image, stream, &wt);
}

extern "C" int gs_photo_loss_weighted_bwd_f64(int64_t batch, int64_t height, int64_t width, int64_t channels,
                                              const double* image, int64_t image_batch_stride,
                                              int64_t image_row_stride, int64_t image_pixel_stride,
                                              const double* target, int64_t target_batch_stride,
                                              int64_t target_row_stride, int64_t target_pixel_stride,
                                              const double* weight, int64_t weight_batch_stride,
                                              int64_t weight_row_stride, int64_t weight_pixel_stride,
                                              const double* normalisers, int32_t window_size, double sigma,
                                              int32_t valid, const double* saved_maps, const double* upstream_map,
                                              const double* grad_loss, double l1_coeff, double ssim_coeff,
                                              double* d_image, void* stream) {
  const LossWeighted<double> wt{weight, weight_batch_stride, weight_row_stride, weight_pixel_stride, normalisers};
  return loss_bwd<double>("gs_photo_loss_weighted_bwd_f64", batch, height, width, channels, image, image_batch_stride,
                          image_row_stride, image_pixel_stride, target, target_batch_stride, target_row_stride,
                          target_pixel_stride, window_size, sigma, valid, saved_maps, upstream_map, grad_loss,
                          l1_coeff, ssim_coeff, d_image, stream, &wt);
}
