// project_math.h -- the projection's per-Gaussian device arithmetic and its adjoint (perspective/projection.py:32-80,
// math in taichi_lib/generic.py:96-158, :217-237, :419-427), written once over the scalar type: project.hip instantiates
// it with float (the training path), project_f64.hip with double (gradcheck and the f64 golden values), so what vouches
// for the formulas in double vouches for the lines the float kernels compile.
//
// The functions below pin their own contraction mode -- `#pragma clang fp contract(fast)` at the head of each body,
// hipcc's default -- so that they produce the same bits whatever the including translation unit's flag says (mapper.hip,
// compiled with -ffp-contract=off, once ran them in a one-pass projection kernel: DESIGN 5).
#pragma once
#include "gs_common.h"
#include "../../include/gs_detmath.h"

#ifdef __HIPCC__
namespace gs_proj {

// The library functions of each scalar type.  float: the deterministic logarithm the mapper shares with the CPU oracle
// (gs_detmath.h); double: IEEE libm.
template <typename Real>
struct Math;
template <>
struct Math<float> {
  static __device__ __forceinline__ float sqrt(float x) { return sqrtf(x); }
  static __device__ __forceinline__ float exp(float x) { return expf(x); }
  static __device__ __forceinline__ float log(float x) { return gs_det_logf(x); }
  static __device__ __forceinline__ float min(float x, float y) { return fminf(x, y); }
  static __device__ __forceinline__ float max(float x, float y) { return fmaxf(x, y); }
};
template <>
struct Math<double> {
  static __device__ __forceinline__ double sqrt(double x) { return ::sqrt(x); }
  static __device__ __forceinline__ double exp(double x) { return ::exp(x); }
  static __device__ __forceinline__ double log(double x) { return ::log(x); }
  static __device__ __forceinline__ double min(double x, double y) { return fmin(x, y); }
  static __device__ __forceinline__ double max(double x, double y) { return fmax(x, y); }
};

template <typename Real>
struct CamT {
  Real T[12];  // rows 0..2 of T_camera_world
  Real fx, fy, cx, cy;
};

template <typename Real>
__device__ __forceinline__ CamT<Real> load_cam(const Real* T44, const Real* proj) {
  CamT<Real> c;
#pragma unroll
  for (int i = 0; i < 12; ++i) c.T[i] = T44[i];
  c.fx = proj[0]; c.fy = proj[1]; c.cx = proj[2]; c.cy = proj[3];
  return c;
}

template <typename Real>
struct ProjArgsT {
  const Real* position;
  const Real* log_scaling;
  const Real* rotation;
  const Real* alpha_logit;
  const Real* T44;
  const Real* proj;
  int64_t n;
  Real width, height, near_p, far_p;
  Real inv_far, ndc_denom;
  Real clamp_margin, blur_cov, alpha_thr;
};

// Everything the forward produces plus the intermediates the adjoint needs.
template <typename Real>
struct FwdT {
  Real qn[4], qlen, s[3];
  Real cam[3];
  Real u, v, tx, ty;
  bool in_x, in_y;
  Real J00, J02, J11, J12;
  Real R[3][3], M3[3][3], N[2][3], m[2][3];
  Real c00, c01, c11, tr, gap, sg, l1, l2, vx, vy, vn;
  Real ax, ay, s1, s2, alpha;
};

using Cam = CamT<float>;
using ProjArgs = ProjArgsT<float>;
using Fwd = FwdT<float>;

template <typename Real>
__device__ __forceinline__ void forward(const ProjArgsT<Real>& a, const CamT<Real>& c, int64_t i, FwdT<Real>& f) {
#pragma clang fp contract(fast)
  using M = Math<Real>;
  const Real* q = a.rotation + 4 * i;
  f.qlen = M::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int k = 0; k < 4; ++k) f.qn[k] = q[k] / f.qlen;
#pragma unroll
  for (int k = 0; k < 3; ++k) f.s[k] = M::exp(a.log_scaling[3 * i + k]);
  const Real px = a.position[3 * i], py = a.position[3 * i + 1], pz = a.position[3 * i + 2];
#pragma unroll
  for (int r = 0; r < 3; ++r) f.cam[r] = c.T[r * 4] * px + c.T[r * 4 + 1] * py + c.T[r * 4 + 2] * pz + c.T[r * 4 + 3];
  const Real z = f.cam[2];
  f.u = (c.fx * f.cam[0]) / z + c.cx;
  f.v = (c.fy * f.cam[1]) / z + c.cy;
  const Real lox = -a.width * a.clamp_margin, hix = (a.width - Real(1)) * (Real(1) + a.clamp_margin);
  const Real loy = -a.height * a.clamp_margin, hiy = (a.height - Real(1)) * (Real(1) + a.clamp_margin);
  f.in_x = f.u >= lox && f.u <= hix;
  f.in_y = f.v >= loy && f.v <= hiy;
  f.tx = M::min(M::max(f.u, lox), hix);
  f.ty = M::min(M::max(f.v, loy), hiy);
  f.J00 = c.fx / z; f.J02 = -(f.tx - c.cx) / z;
  f.J11 = c.fy / z; f.J12 = -(f.ty - c.cy) / z;
  const Real x = f.qn[0], y = f.qn[1], zq = f.qn[2], w = f.qn[3];
  const Real x2 = x * x, y2 = y * y, z2 = zq * zq;
  f.R[0][0] = 1 - 2 * y2 - 2 * z2; f.R[0][1] = 2 * x * y - 2 * w * zq; f.R[0][2] = 2 * x * zq + 2 * w * y;
  f.R[1][0] = 2 * x * y + 2 * w * zq; f.R[1][1] = 1 - 2 * x2 - 2 * z2; f.R[1][2] = 2 * y * zq - 2 * w * x;
  f.R[2][0] = 2 * x * zq - 2 * w * y; f.R[2][1] = 2 * y * zq + 2 * w * x; f.R[2][2] = 1 - 2 * x2 - 2 * y2;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      f.M3[r][k] = c.T[r * 4] * f.R[0][k] + c.T[r * 4 + 1] * f.R[1][k] + c.T[r * 4 + 2] * f.R[2][k];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    f.N[0][k] = f.J00 * f.M3[0][k] + f.J02 * f.M3[2][k];
    f.N[1][k] = f.J11 * f.M3[1][k] + f.J12 * f.M3[2][k];
    f.m[0][k] = f.N[0][k] * f.s[k];
    f.m[1][k] = f.N[1][k] * f.s[k];
  }
  f.c00 = f.m[0][0] * f.m[0][0] + f.m[0][1] * f.m[0][1] + f.m[0][2] * f.m[0][2] + a.blur_cov;
  f.c01 = f.m[0][0] * f.m[1][0] + f.m[0][1] * f.m[1][1] + f.m[0][2] * f.m[1][2];
  f.c11 = f.m[1][0] * f.m[1][0] + f.m[1][1] * f.m[1][1] + f.m[1][2] * f.m[1][2] + a.blur_cov;
  f.tr = f.c00 + f.c11;
  const Real det = f.c00 * f.c11 - f.c01 * f.c01;
  f.gap = f.tr * f.tr - Real(4) * det;
  f.sg = M::sqrt(M::max(f.gap, Real(0)));
  f.l1 = (f.tr + f.sg) * Real(0.5);
  f.l2 = (f.tr - f.sg) * Real(0.5);
  f.vx = f.c00 - f.l2; f.vy = f.c01;
  f.vn = M::sqrt(f.vx * f.vx + f.vy * f.vy);
  f.ax = f.vx / f.vn; f.ay = f.vy / f.vn;
  f.s1 = M::sqrt(f.l1); f.s2 = M::sqrt(f.l2);
  f.alpha = Real(1) / (Real(1) + M::exp(-a.alpha_logit[i]));
}

// camera position = -R^-1 t of the (affine) camera matrix, on the device: CameraParams.camera_position
// (params.py:76-78) without the host round trip of a 4x4 torch.inverse
__device__ __forceinline__ void camera_position(const float* T, float* out) {
#pragma clang fp contract(fast)
  const float a = T[0], b = T[1], c = T[2], d = T[4], e = T[5], f = T[6], g = T[8], h = T[9], i = T[10];
  const float tx = T[3], ty = T[7], tz = T[11];
  const float A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
  const float det = a * A + b * B + c * C;
  const float inv = 1.0f / det;
  // inverse(R) rows
  const float r00 = A * inv, r01 = -(b * i - c * h) * inv, r02 = (b * f - c * e) * inv;
  const float r10 = B * inv, r11 = (a * i - c * g) * inv, r12 = -(a * f - c * d) * inv;
  const float r20 = C * inv, r21 = -(a * h - b * g) * inv, r22 = (a * e - b * d) * inv;
  out[0] = -(r00 * tx + r01 * ty + r02 * tz);
  out[1] = -(r10 * tx + r11 * ty + r12 * tz);
  out[2] = -(r20 * tx + r21 * ty + r22 * tz);
}

// projection.py:60-67: does the Gaussian's alpha_threshold contour reach the image, between the depth planes?  (NaN from
// alpha < threshold fails every comparison)
template <typename Real>
__device__ __forceinline__ bool visible(const ProjArgsT<Real>& a, const FwdT<Real>& f) {
#pragma clang fp contract(fast)
  using M = Math<Real>;
  const Real gs = M::sqrt(Real(2) * M::log(f.alpha / a.alpha_thr));
  const Real sx = f.s1 * gs, sy = f.s2 * gs;
  const Real v1x = f.ax * sx, v1y = f.ay * sx, v2x = -f.ay * sy, v2y = f.ax * sy;
  const Real ex = M::sqrt(v1x * v1x + v2x * v2x), ey = M::sqrt(v1y * v1y + v2y * v2y);
  const Real z = f.cam[2];
  return (z > a.near_p) && (z < a.far_p) && (f.u + ex > Real(0)) && (f.v + ey > Real(0)) && (f.u - ex < a.width) &&
         (f.v - ey < a.height);
}

// ------------------------------------------------------------------------------- backward
template <typename Real>
struct BwdArgsT {
  ProjArgsT<Real> f;
  const int* slot_of;
  const Real* gpoints;  // row stride gpoints_stride, or null
  const Real* gdepth;   // stride gdepth_stride, or null
  const Real* gdepth_sq;  // optional gradient of a z^2 feature (adds 2 z g), same stride as gdepth
  int gpoints_stride, gdepth_stride;
  Real* d_position;
  Real* d_log_scaling;
  Real* d_rotation;
  Real* d_alpha_logit;
  Real* cam_partials;  // (num_blocks,16) or null
};

using BwdArgs = BwdArgsT<float>;

// The adjoint of one visible Gaussian: i = its row in the parameter tensors, slot = its row in the upstream gradients.
// Shared by the dense kernel (one lane per Gaussian) and the row-compact one (one lane per visible row), so that a
// visible row's four gradients are the same bits either way, and by the float64 kernel.  CAMERA: also add this
// Gaussian's share of the camera gradients (T rows 0..2, then fx fy cx cy) into gcam_acc.
template <typename Real, bool CAMERA>
__device__ __forceinline__ void project_bwd_row(const BwdArgsT<Real>& a, const int64_t i, const int slot,
                                                Real (&dpos)[3], Real (&dls)[3], Real (&dq)[4], Real& dal,
                                                Real (&gcam_acc)[16]) {
#pragma clang fp contract(fast)
  const CamT<Real> c = load_cam(a.f.T44, a.f.proj);
  FwdT<Real> f;
  forward(a.f, c, i, f);
  Real g[7] = {0, 0, 0, 0, 0, 0, 0}, gz = Real(0);
  if (a.gpoints) {
#pragma unroll
    for (int k = 0; k < 7; ++k) g[k] = a.gpoints[int64_t(slot) * a.gpoints_stride + k];
  }
  if (a.gdepth) gz = a.gdepth[int64_t(slot) * a.gdepth_stride];
  if (a.gdepth_sq) gz += Real(2) * f.cam[2] * a.gdepth_sq[int64_t(slot) * a.gdepth_stride];
  // alpha = sigmoid(logit)
  dal = g[6] * f.alpha * (Real(1) - f.alpha);
  // sigma = sqrt(lambda)
  Real gl1 = g[4] * Real(0.5) / f.s1, gl2 = g[5] * Real(0.5) / f.s2;
  // axis = v / |v|
  const Real dotag = f.ax * g[2] + f.ay * g[3];
  const Real gvx = (g[2] - f.ax * dotag) / f.vn, gvy = (g[3] - f.ay * dotag) / f.vn;
  Real gc00 = gvx, gc01 = gvy, gc11 = Real(0);
  gl2 -= gvx;
  // lambda1,2 = (tr +- sg)/2
  Real gtr = Real(0.5) * (gl1 + gl2);
  const Real gsg = Real(0.5) * (gl1 - gl2);
  // sg = sqrt(max(gap,0)); at gap == 0 the reference's autodiff yields inf/NaN, we return 0 (DESIGN.md deviation 4)
  const Real ggap = (f.gap > Real(0) && f.sg > Real(0)) ? gsg * Real(0.5) / f.sg : Real(0);
  gtr += Real(2) * f.tr * ggap;
  const Real gdet = Real(-4) * ggap;
  gc00 += gdet * f.c11 + gtr;
  gc11 += gdet * f.c00 + gtr;
  gc01 += Real(-2) * f.c01 * gdet;
  // cov = m m^T
  Real gN[2][3], gs[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const Real gm0 = Real(2) * gc00 * f.m[0][k] + gc01 * f.m[1][k];
    const Real gm1 = Real(2) * gc11 * f.m[1][k] + gc01 * f.m[0][k];
    gs[k] = gm0 * f.N[0][k] + gm1 * f.N[1][k];
    gN[0][k] = gm0 * f.s[k];
    gN[1][k] = gm1 * f.s[k];
    dls[k] = gs[k] * f.s[k];  // s = exp(log_scale)
  }
  // N = J M3
  Real gJ00 = 0, gJ02 = 0, gJ11 = 0, gJ12 = 0, gM3[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    gJ00 += gN[0][k] * f.M3[0][k];
    gJ02 += gN[0][k] * f.M3[2][k];
    gJ11 += gN[1][k] * f.M3[1][k];
    gJ12 += gN[1][k] * f.M3[2][k];
    gM3[0][k] = f.J00 * gN[0][k];
    gM3[1][k] = f.J11 * gN[1][k];
    gM3[2][k] = f.J02 * gN[0][k] + f.J12 * gN[1][k];
  }
  // M3 = Tr R :  gR = Tr^T gM3 ; gTr = gM3 R^T
  Real gR[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      gR[r][k] = c.T[0 * 4 + r] * gM3[0][k] + c.T[1 * 4 + r] * gM3[1][k] + c.T[2 * 4 + r] * gM3[2][k];
      if (CAMERA) gcam_acc[r * 4 + k] += gM3[r][0] * f.R[k][0] + gM3[r][1] * f.R[k][1] + gM3[r][2] * f.R[k][2];
    }
  // R = quat_to_mat(qn)  (generic.py:407-416)
  const Real x = f.qn[0], y = f.qn[1], z = f.qn[2], w = f.qn[3];
  Real gq[4];
  gq[0] = Real(2) * (y * gR[0][1] + z * gR[0][2] + y * gR[1][0] - Real(2) * x * gR[1][1] - w * gR[1][2] + z * gR[2][0] +
                     w * gR[2][1] - Real(2) * x * gR[2][2]);
  gq[1] = Real(2) * (Real(-2) * y * gR[0][0] + x * gR[0][1] + w * gR[0][2] + x * gR[1][0] + z * gR[1][2] - w * gR[2][0] +
                     z * gR[2][1] - Real(2) * y * gR[2][2]);
  gq[2] = Real(2) * (Real(-2) * z * gR[0][0] - w * gR[0][1] + x * gR[0][2] + w * gR[1][0] - Real(2) * z * gR[1][1] +
                     y * gR[1][2] + x * gR[2][0] + y * gR[2][1]);
  gq[3] = Real(2) * (-z * gR[0][1] + y * gR[0][2] + z * gR[1][0] - x * gR[1][2] - y * gR[2][0] + x * gR[2][1]);
  // qn = q / |q|
  const Real dotq = f.qn[0] * gq[0] + f.qn[1] * gq[1] + f.qn[2] * gq[2] + f.qn[3] * gq[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) dq[k] = (gq[k] - f.qn[k] * dotq) / f.qlen;
  // J and the projected mean
  const Real zc = f.cam[2], iz = Real(1) / zc;
  Real gzc = gz;
  Real gfx = gJ00 * iz, gfy = gJ11 * iz;
  gzc += -gJ00 * c.fx * iz * iz - gJ11 * c.fy * iz * iz;
  gzc += gJ02 * (f.tx - c.cx) * iz * iz + gJ12 * (f.ty - c.cy) * iz * iz;
  Real gcx = gJ02 * iz, gcy = gJ12 * iz;
  const Real gu = g[0] + (f.in_x ? -gJ02 * iz : Real(0));  // clamp: zero gradient outside the margin
  const Real gv = g[1] + (f.in_y ? -gJ12 * iz : Real(0));
  gfx += gu * f.cam[0] * iz;
  gfy += gv * f.cam[1] * iz;
  gcx += gu; gcy += gv;
  const Real gcamx = gu * c.fx * iz, gcamy = gv * c.fy * iz;
  gzc += -gu * c.fx * f.cam[0] * iz * iz - gv * c.fy * f.cam[1] * iz * iz;
  // cam = Tr p + t
  const Real gcamv[3] = {gcamx, gcamy, gzc};
  const Real px = a.f.position[3 * i], py = a.f.position[3 * i + 1], pz = a.f.position[3 * i + 2];
#pragma unroll
  for (int k = 0; k < 3; ++k) dpos[k] = c.T[0 * 4 + k] * gcamv[0] + c.T[1 * 4 + k] * gcamv[1] + c.T[2 * 4 + k] * gcamv[2];
  if (CAMERA) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      gcam_acc[r * 4 + 0] += gcamv[r] * px;
      gcam_acc[r * 4 + 1] += gcamv[r] * py;
      gcam_acc[r * 4 + 2] += gcamv[r] * pz;
      gcam_acc[r * 4 + 3] += gcamv[r];
    }
    gcam_acc[12] = gfx; gcam_acc[13] = gfy; gcam_acc[14] = gcx; gcam_acc[15] = gcy;
  }
}

}  // namespace gs_proj
#endif
