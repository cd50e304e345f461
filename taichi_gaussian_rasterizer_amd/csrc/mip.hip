// mip.hip -- the 3D smoothing filter of Mip-Splatting: the per-Gaussian sampling rate over a set of training cameras,
// and the low-pass of (log_scaling, alpha_logit) with its dense and row-compact backward.
//
// SAMPLING RATE.  One lane per point, the point in registers, a loop over the packed camera table.  The camera index is
// the loop counter (the same in every lane), the table a const __restrict__ pointer: the 24 floats of a record arrive by
// scalar loads and sit in SGPRs, so the loop body is VALU only.  Per pair, in float32, every product and sum rounded on
// its own (the unit is compiled with -ffp-contract=off):
//   xc = ((T00*px + T01*py) + T02*pz) + T03      (yc, zc from rows 1, 2)
//   u  = fx*xc + cx*zc     v = fy*yc + cy*zc
//   valid = zc >= near && zc <= far && lo_x*zc <= u && u <= hi_x*zc && lo_y*zc <= v && v <= hi_y*zc
//   rate  = max over the valid cameras of focal / zc (IEEE division), seen = their number
// The division runs under the valid branch only: most (point, camera) pairs of a real capture are outside the frustum.
// A maximum of exactly defined values does not depend on the order, so the result repeats bit for bit and equals a
// float32 restatement on the host.  A NaN fails every comparison: a non-finite point is never valid.
//
// SMOOTHING.  scale' = sqrt(scale^2 + f^2), opacity' = opacity * sqrt(det S / det S'), in the parametrisation Gaussians3D
// stores.  With t = f e^{-l}, x = t^2:
//   x <= 1:  L = log1p(x),              l' = l + L / 2
//   x >  1:  w = log1p(1 / x),          l' = log f + w / 2,   L = 2 log t + w     (x may overflow to inf: 1 / x = 0)
//   log c = -(L_0 + L_1 + L_2) / 2,   1 - c = -expm1(log c),   q = e^a (1 - c)
//   q <= 1:  a' = a + log c - log1p(q)        q > 1:  a' = log c - log(e^{-a} + (1 - c))
// and for the backward r = 1 / (1 + x), s = x / (1 + x) from x or from 1 / x, whichever is <= 1, and
//   1 / (1 - sigmoid(a) c) = (1 + e^a) / (1 + q) = (e^{-a} + 1) / (e^{-a} + (1 - c)),   da'/da = 1 / (1 + q)
// in the form whose exponential is <= 1.  Nothing is saved by the forward: the backward recomputes from (l, a, f).
// A row with f == 0 is copied: outputs and gradients keep their bits.  The dense and the row-compact backward call the
// same device function, and without contraction the same instructions: their rows agree bit for bit.

#include <math.h>

#include "gs_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;

// ------------------------------------------------------------------------------------------------- sampling rate
__global__ __launch_bounds__(kThreads) void mip_rate_kernel(int n, const float* __restrict__ position, int cameras,
                                                            const float* __restrict__ packed, float* __restrict__ rate,
                                                            int32_t* __restrict__ seen) {
  const int i = blockIdx.x * kThreads + threadIdx.x;  // n < 2^31 and the grid is ceil(n / 256): no overflow
  if (i >= n) return;
  const float px = position[3 * int64_t(i)], py = position[3 * int64_t(i) + 1], pz = position[3 * int64_t(i) + 2];
  float best = 0.0f;
  int count = 0;
  for (int c = 0; c < cameras; ++c) {
    // uniform index: scalar loads.  The whole record is read in front of the arithmetic (no load behind a branch)
    float cam[GS_MIP_CAMERA_FLOATS - 1];
#pragma unroll
    for (int k = 0; k < GS_MIP_CAMERA_FLOATS - 1; ++k) cam[k] = packed[c * GS_MIP_CAMERA_FLOATS + k];
    float focal = cam[22];
    asm volatile("" : "+s"(focal));  // in an SGPR here: the compiler would sink this one load into the branch
    const float xc = ((cam[0] * px + cam[1] * py) + cam[2] * pz) + cam[3];
    const float yc = ((cam[4] * px + cam[5] * py) + cam[6] * pz) + cam[7];
    const float zc = ((cam[8] * px + cam[9] * py) + cam[10] * pz) + cam[11];
    const float u = cam[12] * xc + cam[14] * zc;
    const float v = cam[13] * yc + cam[15] * zc;
    // & not &&: six compares and five mask operations, one branch
    const bool valid = bool(int(zc >= cam[20]) & int(zc <= cam[21]) & int(cam[16] * zc <= u) & int(u <= cam[17] * zc) &
                            int(cam[18] * zc <= v) & int(v <= cam[19] * zc));
    if (valid) {
      best = fmaxf(best, __fdiv_rn(focal, zc));  // zc >= near: never NaN unless near is
      ++count;
    }
  }
  rate[i] = best;
  seen[i] = count;
}

// ----------------------------------------------------------------------------------------------------- smoothing
__device__ __forceinline__ float m_exp(float x) { return expf(x); }
__device__ __forceinline__ double m_exp(double x) { return exp(x); }
__device__ __forceinline__ float m_log(float x) { return logf(x); }
__device__ __forceinline__ double m_log(double x) { return log(x); }
__device__ __forceinline__ float m_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ double m_log1p(double x) { return log1p(x); }
__device__ __forceinline__ float m_expm1(float x) { return expm1f(x); }
__device__ __forceinline__ double m_expm1(double x) { return expm1(x); }

// what forward and backward share: per axis x (or 1 / x) and the smoothed log scale, and log c
template <typename T>
struct Smooth {
  T lp[3];    // l'
  T r[3];     // 1 / (1 + x)
  T s[3];     // x / (1 + x)
  T log_c;
};

template <typename T>
__device__ __forceinline__ Smooth<T> smooth_terms(const T l[3], T f) {
  Smooth<T> o;
  const T log_f = m_log(f);
  T sum = T(0);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const T t = f * m_exp(-l[k]);
    const T x = t * t;
    if (x <= T(1)) {
      const T L = m_log1p(x);
      o.lp[k] = l[k] + T(0.5) * L;
      o.r[k] = T(1) / (T(1) + x);
      o.s[k] = x * o.r[k];
      sum += L;
    } else {  // also x = inf
      const T y = T(1) / x;
      const T w = m_log1p(y);
      o.lp[k] = log_f + T(0.5) * w;
      o.s[k] = T(1) / (T(1) + y);
      o.r[k] = y * o.s[k];
      sum += T(2) * m_log(t) + w;
    }
  }
  o.log_c = T(-0.5) * sum;
  return o;
}

template <typename T>
__device__ __forceinline__ void smooth_fwd_row(const T l[3], T a, T f, T out_l[3], T& out_a) {
  if (f == T(0)) {
    out_l[0] = l[0]; out_l[1] = l[1]; out_l[2] = l[2];
    out_a = a;
    return;
  }
  const Smooth<T> o = smooth_terms(l, f);
  out_l[0] = o.lp[0]; out_l[1] = o.lp[1]; out_l[2] = o.lp[2];
  const T omc = -m_expm1(o.log_c);  // 1 - c
  const T q = m_exp(a) * omc;
  if (q <= T(1))
    out_a = (a + o.log_c) - m_log1p(q);
  else
    out_a = o.log_c - m_log(m_exp(-a) + omc);
}

// THE backward of one row, for the dense and the row-compact kernel alike
template <typename T>
__device__ __forceinline__ void smooth_bwd_row(const T l[3], T a, T f, const T gl[3], T ga, T dl[3], T& da) {
  if (f == T(0)) {
    dl[0] = gl[0]; dl[1] = gl[1]; dl[2] = gl[2];
    da = ga;
    return;
  }
  const Smooth<T> o = smooth_terms(l, f);
  const T omc = -m_expm1(o.log_c);
  T inv_rest, da_da;  // 1 / (1 - sigmoid(a) c), da'/da
  if (a <= T(0)) {
    const T e = m_exp(a), q1 = T(1) + e * omc;
    inv_rest = (T(1) + e) / q1;
    da_da = T(1) / q1;
  } else {
    const T em = m_exp(-a), den = em + omc;
    inv_rest = (em + T(1)) / den;
    da_da = em / den;
  }
  const T through_a = ga * inv_rest;
#pragma unroll
  for (int k = 0; k < 3; ++k) dl[k] = gl[k] * o.r[k] + through_a * o.s[k];
  da = ga * da_da;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void smooth_fwd_kernel(int n, const T* __restrict__ log_scaling,
                                                              const T* __restrict__ alpha_logit,
                                                              const T* __restrict__ filter3d, T* __restrict__ out_l,
                                                              T* __restrict__ out_a) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t at = 3 * int64_t(i);
  const T l[3] = {log_scaling[at], log_scaling[at + 1], log_scaling[at + 2]};
  T ol[3], oa;
  smooth_fwd_row<T>(l, alpha_logit[i], filter3d[i], ol, oa);
  out_l[at] = ol[0]; out_l[at + 1] = ol[1]; out_l[at + 2] = ol[2];
  out_a[i] = oa;
}

// rows == NULL: the dense form, gradient row i belongs to parameter row i.  Otherwise gradient row i belongs to
// parameter row rows[i]; a row index outside [0, n) gives a zero gradient row and reads nothing.
template <typename T>
__global__ __launch_bounds__(kThreads) void smooth_bwd_kernel(int n, int v, const int64_t* __restrict__ rows,
                                                              const T* __restrict__ log_scaling,
                                                              const T* __restrict__ alpha_logit,
                                                              const T* __restrict__ filter3d, const T* __restrict__ grad_l,
                                                              const T* __restrict__ grad_a, T* __restrict__ d_l,
                                                              T* __restrict__ d_a) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= v) return;
  const int64_t g = 3 * int64_t(i);
  int64_t row = i;
  if (rows) {
    row = rows[i];
    if (row < 0 || row >= n) {
      d_l[g] = T(0); d_l[g + 1] = T(0); d_l[g + 2] = T(0);
      d_a[i] = T(0);
      return;
    }
  }
  const int64_t at = 3 * row;
  const T l[3] = {log_scaling[at], log_scaling[at + 1], log_scaling[at + 2]};
  T gl[3] = {T(0), T(0), T(0)}, ga = T(0);
  if (grad_l) { gl[0] = grad_l[g]; gl[1] = grad_l[g + 1]; gl[2] = grad_l[g + 2]; }
  if (grad_a) ga = grad_a[i];
  T dl[3], da;
  smooth_bwd_row<T>(l, alpha_logit[row], filter3d[row], gl, ga, dl, da);
  d_l[g] = dl[0]; d_l[g + 1] = dl[1]; d_l[g + 2] = dl[2];
  d_a[i] = da;
}

// ---------------------------------------------------------------------------------------------------- host checks
bool aligned(const void* p, size_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }

int check_rows(const char* what, int64_t n) {
  GS_REQUIRE(n >= 0 && n < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT, "%s: %lld rows (0 .. 2^31 - 1)", what,
             (long long)n);
  return GS_OK;
}

// every named buffer non-NULL (unless optional) and aligned to its element
struct Buf {
  const char* name;
  const void* p;
  bool optional;
};
int check_bufs(const char* what, const Buf* bufs, int count, size_t elem) {
  for (int b = 0; b < count; ++b) {
    GS_REQUIRE(bufs[b].p || bufs[b].optional, GS_ERR_INVALID_ARGUMENT, "%s: NULL buffer (%s)", what, bufs[b].name);
    GS_REQUIRE(aligned(bufs[b].p, elem), GS_ERR_INVALID_ARGUMENT, "%s: %s is not %d-byte aligned", what, bufs[b].name,
               int(elem));
  }
  return GS_OK;
}

template <typename T>
int smooth_fwd(const char* what, int64_t n, const T* l, const T* a, const T* f, T* out_l, T* out_a, void* stream) {
  if (int rc = check_rows(what, n)) return rc;
  if (n == 0) return GS_OK;
  const Buf bufs[] = {{"log_scaling", l, false}, {"alpha_logit", a, false}, {"filter3d", f, false},
                      {"out_log_scaling", out_l, false}, {"out_alpha_logit", out_a, false}};
  if (int rc = check_bufs(what, bufs, 5, sizeof(T))) return rc;
  hipLaunchKernelGGL(smooth_fwd_kernel<T>, dim3(unsigned(gs_div_up(n, kThreads))), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), int(n), l, a, f, out_l, out_a);
  GS_CHECK_LAUNCH(what);
  return GS_OK;
}

template <typename T>
int smooth_bwd(const char* what, int64_t n, int64_t v, bool by_rows, const int64_t* rows, const T* l, const T* a,
               const T* f, const T* grad_l, const T* grad_a, T* d_l, T* d_a, void* stream) {
  if (int rc = check_rows(what, n)) return rc;
  if (by_rows)
    GS_REQUIRE(v >= 0 && v < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT, "%s: %lld gradient rows (0 .. 2^31 - 1)", what,
               (long long)v);
  if (v == 0) return GS_OK;
  GS_REQUIRE(n > 0, GS_ERR_INVALID_ARGUMENT, "%s: %lld gradient rows of an empty table", what, (long long)v);
  if (by_rows) {
    GS_REQUIRE(rows, GS_ERR_INVALID_ARGUMENT, "%s: NULL buffer (rows)", what);
    GS_REQUIRE(aligned(rows, 8), GS_ERR_INVALID_ARGUMENT, "%s: rows is not 8-byte aligned", what);
  }
  const Buf bufs[] = {{"log_scaling", l, false}, {"alpha_logit", a, false}, {"filter3d", f, false},
                      {"grad_log_scaling", grad_l, true}, {"grad_alpha_logit", grad_a, true},
                      {"d_log_scaling", d_l, false}, {"d_alpha_logit", d_a, false}};
  if (int rc = check_bufs(what, bufs, 7, sizeof(T))) return rc;
  hipLaunchKernelGGL(smooth_bwd_kernel<T>, dim3(unsigned(gs_div_up(v, kThreads))), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), int(n), int(v), rows, l, a, f, grad_l, grad_a, d_l, d_a);
  GS_CHECK_LAUNCH(what);
  return GS_OK;
}

}  // namespace

extern "C" int gs_mip_sampling_rate(int64_t n, const float* position, int32_t cameras, const float* packed, float* rate,
                                    int32_t* seen, void* stream) {
  const char* what = "gs_mip_sampling_rate";
  if (int rc = check_rows(what, n)) return rc;
  GS_REQUIRE(cameras >= 0 && cameras <= GS_MIP_CAMERAS_MAX, GS_ERR_INVALID_ARGUMENT, "%s: %d cameras (0 .. %d)", what,
             cameras, GS_MIP_CAMERAS_MAX);
  if (n == 0) return GS_OK;
  const Buf bufs[] = {{"position", position, false}, {"packed", packed, cameras == 0}, {"rate", rate, false},
                      {"seen", seen, false}};
  if (int rc = check_bufs(what, bufs, 4, 4)) return rc;
  hipLaunchKernelGGL(mip_rate_kernel, dim3(unsigned(gs_div_up(n, kThreads))), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), int(n), position, int(cameras), packed, rate, seen);
  GS_CHECK_LAUNCH(what);
  return GS_OK;
}

extern "C" int gs_smooth3d_fwd(int64_t n, const float* log_scaling, const float* alpha_logit, const float* filter3d,
                               float* out_log_scaling, float* out_alpha_logit, void* stream) {
  return smooth_fwd<float>("gs_smooth3d_fwd", n, log_scaling, alpha_logit, filter3d, out_log_scaling, out_alpha_logit,
                           stream);
}

extern "C" int gs_smooth3d_fwd_f64(int64_t n, const double* log_scaling, const double* alpha_logit,
                                   const double* filter3d, double* out_log_scaling, double* out_alpha_logit,
                                   void* stream) {
  return smooth_fwd<double>("gs_smooth3d_fwd_f64", n, log_scaling, alpha_logit, filter3d, out_log_scaling,
                            out_alpha_logit, stream);
}

extern "C" int gs_smooth3d_bwd(int64_t n, const float* log_scaling, const float* alpha_logit, const float* filter3d,
                               const float* grad_log_scaling, const float* grad_alpha_logit, float* d_log_scaling,
                               float* d_alpha_logit, void* stream) {
  return smooth_bwd<float>("gs_smooth3d_bwd", n, n, false, nullptr, log_scaling, alpha_logit, filter3d,
                           grad_log_scaling, grad_alpha_logit, d_log_scaling, d_alpha_logit, stream);
}

extern "C" int gs_smooth3d_bwd_f64(int64_t n, const double* log_scaling, const double* alpha_logit,
                                   const double* filter3d, const double* grad_log_scaling,
                                   const double* grad_alpha_logit, double* d_log_scaling, double* d_alpha_logit,
                                   void* stream) {
  return smooth_bwd<double>("gs_smooth3d_bwd_f64", n, n, false, nullptr, log_scaling, alpha_logit, filter3d,
                            grad_log_scaling, grad_alpha_logit, d_log_scaling, d_alpha_logit, stream);
}

extern "C" int gs_smooth3d_bwd_rows(int64_t n, int64_t v, const int64_t* rows, const float* log_scaling,
                                    const float* alpha_logit, const float* filter3d, const float* grad_log_scaling,
                                    const float* grad_alpha_logit, float* d_log_scaling, float* d_alpha_logit,
                                    void* stream) {
  return smooth_bwd<float>("gs_smooth3d_bwd_rows", n, v, true, rows, log_scaling, alpha_logit, filter3d,
                           grad_log_scaling, grad_alpha_logit, d_log_scaling, d_alpha_logit, stream);
}
