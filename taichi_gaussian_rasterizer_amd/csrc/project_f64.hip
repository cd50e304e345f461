// project_f64.hip -- the perspective projection and its adjoint in float64, for gradcheck.  The arithmetic of
// project_math.h / project.hip (perspective/projection.py:32-80, taichi_lib/generic.py:96-158, :217-237, :419-427)
// restated in double with IEEE sqrt / exp / log and double constants; the f32 path keeps its own translation units
// untouched.  As in f32, a zero eigen-gap gives a zero adjoint (DESIGN.md deviation 4), and the camera gradients are
// per-workgroup partials reduced in a fixed order.

#include "f64_common.h"

namespace {

struct Args {
  const double* position;
  const double* log_scaling;
  const double* rotation;
  const double* alpha_logit;
  const double* T44;
  const double* proj;
  int64_t n;
  double width, height, near_p, far_p;
  double clamp_margin, blur_cov, alpha_thr;
};

struct Fwd {
  double qn[4], qlen, s[3];
  double cam[3];
  double u, v, tx, ty;
  bool in_x, in_y;
  double J00, J02, J11, J12;
  double R[3][3], M3[3][3], N[2][3], m[2][3];
  double c00, c01, c11, tr, gap, sg, l1, l2, vx, vy, vn;
  double ax, ay, s1, s2, alpha;
};

__device__ __forceinline__ void forward(const Args& a, int64_t i, Fwd& f) {
  const double* T = a.T44;
  const double fx = a.proj[0], fy = a.proj[1], cx = a.proj[2], cy = a.proj[3];
  const double* q = a.rotation + 4 * i;
  f.qlen = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; ++k) f.qn[k] = q[k] / f.qlen;
  for (int k = 0; k < 3; ++k) f.s[k] = exp(a.log_scaling[3 * i + k]);
  const double px = a.position[3 * i], py = a.position[3 * i + 1], pz = a.position[3 * i + 2];
  for (int r = 0; r < 3; ++r) f.cam[r] = T[r * 4] * px + T[r * 4 + 1] * py + T[r * 4 + 2] * pz + T[r * 4 + 3];
  const double z = f.cam[2];
  f.u = (fx * f.cam[0]) / z + cx;
  f.v = (fy * f.cam[1]) / z + cy;
  const double lox = -a.width * a.clamp_margin, hix = (a.width - 1.0) * (1.0 + a.clamp_margin);
  const double loy = -a.height * a.clamp_margin, hiy = (a.height - 1.0) * (1.0 + a.clamp_margin);
  f.in_x = f.u >= lox && f.u <= hix;
  f.in_y = f.v >= loy && f.v <= hiy;
  f.tx = f.u < lox ? lox : (f.u > hix ? hix : f.u);
  f.ty = f.v < loy ? loy : (f.v > hiy ? hiy : f.v);
  f.J00 = fx / z; f.J02 = -(f.tx - cx) / z;
  f.J11 = fy / z; f.J12 = -(f.ty - cy) / z;
  const double x = f.qn[0], y = f.qn[1], zq = f.qn[2], w = f.qn[3];
  const double x2 = x * x, y2 = y * y, z2 = zq * zq;
  f.R[0][0] = 1 - 2 * y2 - 2 * z2; f.R[0][1] = 2 * x * y - 2 * w * zq; f.R[0][2] = 2 * x * zq + 2 * w * y;
  f.R[1][0] = 2 * x * y + 2 * w * zq; f.R[1][1] = 1 - 2 * x2 - 2 * z2; f.R[1][2] = 2 * y * zq - 2 * w * x;
  f.R[2][0] = 2 * x * zq - 2 * w * y; f.R[2][1] = 2 * y * zq + 2 * w * x; f.R[2][2] = 1 - 2 * x2 - 2 * y2;
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) f.M3[r][k] = T[r * 4] * f.R[0][k] + T[r * 4 + 1] * f.R[1][k] + T[r * 4 + 2] * f.R[2][k];
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
  const double det = f.c00 * f.c11 - f.c01 * f.c01;
  f.gap = f.tr * f.tr - 4.0 * det;
  f.sg = sqrt(f.gap > 0.0 ? f.gap : 0.0);
  f.l1 = (f.tr + f.sg) * 0.5;
  f.l2 = (f.tr - f.sg) * 0.5;
  f.vx = f.c00 - f.l2; f.vy = f.c01;
  f.vn = sqrt(f.vx * f.vx + f.vy * f.vy);
  f.ax = f.vx / f.vn; f.ay = f.vy / f.vn;
  f.s1 = sqrt(f.l1); f.s2 = sqrt(f.l2);
  f.alpha = 1.0 / (1.0 + exp(-a.alpha_logit[i]));
}

// projection.py:60-67 (NaN from alpha < threshold fails every comparison)
__device__ __forceinline__ bool visible(const Args& a, const Fwd& f) {
  const double gs = sqrt(2.0 * log(f.alpha / a.alpha_thr));
  const double sx = f.s1 * gs, sy = f.s2 * gs;
  const double v1x = f.ax * sx, v1y = f.ay * sx, v2x = -f.ay * sy, v2y = f.ax * sy;
  const double ex = sqrt(v1x * v1x + v2x * v2x), ey = sqrt(v1y * v1y + v2y * v2y);
  const double z = f.cam[2];
  return (z > a.near_p) && (z < a.far_p) && (f.u + ex > 0.0) && (f.u - ex < a.width) && (f.v + ey > 0.0) &&
         (f.v - ey < a.height);
}

// pass 1: project, stage the row [points(7), depth], count the visible per workgroup
__global__ __launch_bounds__(256) void project_f64_kernel(Args a, double* st_rows, int32_t* flags,
                                                          int32_t* block_counts) {
  __shared__ int32_t s_cnt[4];
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  bool vis = false;
  if (i < a.n) {
    Fwd f;
    forward(a, i, f);
    vis = visible(a, f);
    double* r = st_rows + 8 * i;
    r[0] = f.u; r[1] = f.v; r[2] = f.ax; r[3] = f.ay; r[4] = f.s1; r[5] = f.s2; r[6] = f.alpha; r[7] = f.cam[2];
    flags[i] = vis ? 1 : 0;
  }
  const uint64_t b = __ballot(vis);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// pass 2: stable compaction behind the scanned workgroup counts (offsets: nb + 1 entries, offsets[nb] = total)
__global__ __launch_bounds__(256) void compact_f64_kernel(int64_t n, int nb, const double* st_rows,
                                                          const int32_t* flags, const int32_t* offsets, double inv_far,
                                                          double ndc_denom, double* points, double* depth, double* ndc,
                                                          int64_t* indexes, int32_t* slot_of, int32_t* num_visible) {
  __shared__ int32_t s_cnt[4];
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const bool vis = i < n && flags[i] != 0;
  const uint64_t b = __ballot(vis);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) s_cnt[wave] = __popcll(b);
  __syncthreads();
  int base = offsets[blockIdx.x];
  for (int w = 0; w < wave; ++w) base += s_cnt[w];
  if (i < n) {
    int slot = -1;
    if (vis) {
      slot = base + __popcll(b & ((1ull << lane) - 1ull));
      const double* r = st_rows + 8 * i;
      for (int k = 0; k < 7; ++k) points[int64_t(slot) * 7 + k] = r[k];
      depth[slot] = r[7];
      ndc[slot] = 1.0 - (1.0 / r[7] - inv_far) / ndc_denom;  // torch_lib/projection.py:120-123
      indexes[slot] = i;
    }
    slot_of[i] = slot;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *num_visible = offsets[nb];
}

struct BwdArgs {
  Args f;
  const int32_t* slot_of;
  const double* gpoints;  // (V,7) or null
  const double* gdepth;   // (V) or null
  double* d_position;
  double* d_log_scaling;
  double* d_rotation;
  double* d_alpha_logit;
  double* cam_partials;  // (num_blocks,16) or null
};

// the adjoint of forward(): project.hip project_bwd_kernel in double
__global__ __launch_bounds__(256) void project_bwd_f64_kernel(BwdArgs a) {
  __shared__ double s_red[4];
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  double gcam[16];
  for (int k = 0; k < 16; ++k) gcam[k] = 0.0;
  const int slot = i < a.f.n ? a.slot_of[i] : -1;
  if (i < a.f.n) {
    double dpos[3] = {0, 0, 0}, dls[3] = {0, 0, 0}, dq[4] = {0, 0, 0, 0}, dal = 0;
    if (slot >= 0) {
      const double* T = a.f.T44;
      const double fx = a.f.proj[0], fy = a.f.proj[1], cx = a.f.proj[2], cy = a.f.proj[3];
      Fwd f;
      forward(a.f, i, f);
      double g[7] = {0, 0, 0, 0, 0, 0, 0}, gz = 0.0;
      if (a.gpoints)
        for (int k = 0; k < 7; ++k) g[k] = a.gpoints[int64_t(slot) * 7 + k];
      if (a.gdepth) gz = a.gdepth[slot];
      dal = g[6] * f.alpha * (1.0 - f.alpha);  // alpha = sigmoid(logit)
      double gl1 = g[4] * 0.5 / f.s1, gl2 = g[5] * 0.5 / f.s2;  // sigma = sqrt(lambda)
      const double dotag = f.ax * g[2] + f.ay * g[3];  // axis = v / |v|
      const double gvx = (g[2] - f.ax * dotag) / f.vn, gvy = (g[3] - f.ay * dotag) / f.vn;
      double gc00 = gvx, gc01 = gvy, gc11 = 0.0;
      gl2 -= gvx;
      double gtr = 0.5 * (gl1 + gl2);  // lambda1,2 = (tr +- sg)/2
      const double gsg = 0.5 * (gl1 - gl2);
      const double ggap = (f.gap > 0.0 && f.sg > 0.0) ? gsg * 0.5 / f.sg : 0.0;  // zero eigen-gap: 0 (deviation 4)
      gtr += 2.0 * f.tr * ggap;
      const double gdet = -4.0 * ggap;
      gc00 += gdet * f.c11 + gtr;
      gc11 += gdet * f.c00 + gtr;
      gc01 += -2.0 * f.c01 * gdet;
      double gN[2][3];
      for (int k = 0; k < 3; ++k) {  // cov = m m^T, m = N s
        const double gm0 = 2.0 * gc00 * f.m[0][k] + gc01 * f.m[1][k];
        const double gm1 = 2.0 * gc11 * f.m[1][k] + gc01 * f.m[0][k];
        const double gs = gm0 * f.N[0][k] + gm1 * f.N[1][k];
        gN[0][k] = gm0 * f.s[k];
        gN[1][k] = gm1 * f.s[k];
        dls[k] = gs * f.s[k];  // s = exp(log_scale)
      }
      double gJ00 = 0, gJ02 = 0, gJ11 = 0, gJ12 = 0, gM3[3][3];
      for (int k = 0; k < 3; ++k) {  // N = J M3
        gJ00 += gN[0][k] * f.M3[0][k];
        gJ02 += gN[0][k] * f.M3[2][k];
        gJ11 += gN[1][k] * f.M3[1][k];
        gJ12 += gN[1][k] * f.M3[2][k];
        gM3[0][k] = f.J00 * gN[0][k];
        gM3[1][k] = f.J11 * gN[1][k];
        gM3[2][k] = f.J02 * gN[0][k] + f.J12 * gN[1][k];
      }
      double gR[3][3];
      for (int r = 0; r < 3; ++r)  // M3 = Tr R
        for (int k = 0; k < 3; ++k) {
          gR[r][k] = T[0 * 4 + r] * gM3[0][k] + T[1 * 4 + r] * gM3[1][k] + T[2 * 4 + r] * gM3[2][k];
          gcam[r * 4 + k] += gM3[r][0] * f.R[k][0] + gM3[r][1] * f.R[k][1] + gM3[r][2] * f.R[k][2];
        }
      const double x = f.qn[0], y = f.qn[1], z = f.qn[2], w = f.qn[3];  // R = quat_to_mat(qn)
      double gq[4];
      gq[0] = 2.0 * (y * gR[0][1] + z * gR[0][2] + y * gR[1][0] - 2.0 * x * gR[1][1] - w * gR[1][2] + z * gR[2][0] +
                     w * gR[2][1] - 2.0 * x * gR[2][2]);
      gq[1] = 2.0 * (-2.0 * y * gR[0][0] + x * gR[0][1] + w * gR[0][2] + x * gR[1][0] + z * gR[1][2] - w * gR[2][0] +
                     z * gR[2][1] - 2.0 * y * gR[2][2]);
      gq[2] = 2.0 * (-2.0 * z * gR[0][0] - w * gR[0][1] + x * gR[0][2] + w * gR[1][0] - 2.0 * z * gR[1][1] +
                     y * gR[1][2] + x * gR[2][0] + y * gR[2][1]);
      gq[3] = 2.0 * (-z * gR[0][1] + y * gR[0][2] + z * gR[1][0] - x * gR[1][2] - y * gR[2][0] + x * gR[2][1]);
      const double dotq = f.qn[0] * gq[0] + f.qn[1] * gq[1] + f.qn[2] * gq[2] + f.qn[3] * gq[3];  // qn = q / |q|
      for (int k = 0; k < 4; ++k) dq[k] = (gq[k] - f.qn[k] * dotq) / f.qlen;
      const double zc = f.cam[2], iz = 1.0 / zc;  // J and the projected mean
      double gzc = gz;
      double gfx = gJ00 * iz, gfy = gJ11 * iz;
      gzc += -gJ00 * fx * iz * iz - gJ11 * fy * iz * iz;
      gzc += gJ02 * (f.tx - cx) * iz * iz + gJ12 * (f.ty - cy) * iz * iz;
      double gcx = gJ02 * iz, gcy = gJ12 * iz;
      const double gu = g[0] + (f.in_x ? -gJ02 * iz : 0.0);  // clamp: zero gradient outside the margin
      const double gv = g[1] + (f.in_y ? -gJ12 * iz : 0.0);
      gfx += gu * f.cam[0] * iz;
      gfy += gv * f.cam[1] * iz;
      gcx += gu; gcy += gv;
      const double gcamv[3] = {gu * fx * iz, gv * fy * iz,
                               gzc - gu * fx * f.cam[0] * iz * iz - gv * fy * f.cam[1] * iz * iz};
      const double px = a.f.position[3 * i], py = a.f.position[3 * i + 1], pz = a.f.position[3 * i + 2];
      for (int k = 0; k < 3; ++k) dpos[k] = T[0 * 4 + k] * gcamv[0] + T[1 * 4 + k] * gcamv[1] + T[2 * 4 + k] * gcamv[2];
      for (int r = 0; r < 3; ++r) {  // cam = Tr p + t
        gcam[r * 4 + 0] += gcamv[r] * px;
        gcam[r * 4 + 1] += gcamv[r] * py;
        gcam[r * 4 + 2] += gcamv[r] * pz;
        gcam[r * 4 + 3] += gcamv[r];
      }
      gcam[12] = gfx; gcam[13] = gfy; gcam[14] = gcx; gcam[15] = gcy;
    }
    for (int k = 0; k < 3; ++k) a.d_position[3 * i + k] = dpos[k];
    for (int k = 0; k < 3; ++k) a.d_log_scaling[3 * i + k] = dls[k];
    for (int k = 0; k < 4; ++k) a.d_rotation[4 * i + k] = dq[k];
    a.d_alpha_logit[i] = dal;
  }
  if (a.cam_partials) {
    for (int k = 0; k < 16; ++k) {
      const double t = gs_f64_block_sum<4>(gcam[k], s_red);
      if (threadIdx.x == 0) a.cam_partials[int64_t(blockIdx.x) * 16 + k] = t;
    }
  }
}

// the workgroups' camera partials in a fixed order: strided per lane, then a fixed tree
__global__ __launch_bounds__(256) void cam_reduce_f64_kernel(int num_blocks, const double* partials, double* dT44,
                                                             double* dproj) {
  __shared__ double s_red[4];
  for (int k = 0; k < 16; ++k) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < num_blocks; b += 256) acc += partials[int64_t(b) * 16 + k];
    const double t = gs_f64_block_sum<4>(acc, s_red);
    if (threadIdx.x == 0) {
      if (k < 12) { if (dT44) dT44[k] = t; }
      else if (dproj) dproj[k - 12] = t;
    }
  }
  if (threadIdx.x < 4 && dT44) dT44[12 + threadIdx.x] = 0.0;
}

int fill(Args& a, int64_t n, const double* position, const double* log_scaling, const double* rotation,
         const double* alpha_logit, const double* T, const double* proj, int width, int height, double near_p,
         double far_p, const GsRasterConfigF64* cfg, const char* what) {
  GS_REQUIRE(cfg != nullptr, GS_ERR_INVALID_ARGUMENT, "%s: config is NULL", what);
  GS_REQUIRE(cfg->alpha_threshold > 0.0, GS_ERR_INVALID_ARGUMENT, "%s: alpha_threshold must be > 0", what);
  GS_REQUIRE(n >= 0 && n < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT, "%s: %lld gaussians", what, (long long)n);
  GS_REQUIRE(width > 0 && height > 0, GS_ERR_INVALID_ARGUMENT, "%s: image size %dx%d", what, width, height);
  GS_REQUIRE(n == 0 || (position && log_scaling && rotation && alpha_logit), GS_ERR_INVALID_ARGUMENT,
             "%s: NULL gaussian tensor", what);
  GS_REQUIRE(T && proj, GS_ERR_INVALID_ARGUMENT, "%s: NULL camera", what);
  a.position = position; a.log_scaling = log_scaling; a.rotation = rotation; a.alpha_logit = alpha_logit;
  a.T44 = T; a.proj = proj; a.n = n;
  a.width = double(width); a.height = double(height);
  a.near_p = near_p; a.far_p = far_p;
  a.clamp_margin = cfg->clamp_margin; a.blur_cov = cfg->blur_cov; a.alpha_thr = cfg->alpha_threshold;
  return GS_OK;
}

}  // namespace

extern "C" int64_t gs_project_f64_scratch_bytes(int64_t n) {
  const int64_t nb = gs_div_up(n, 256);
  return gs_align_up(n * 64, 256) + gs_align_up(n * 4, 256) + gs_align_up((nb + 1) * 4, 256) * 2 +
         gs_cumsum_scratch_bytes(nb) + 256;
}

extern "C" int gs_project_fwd_f64(int64_t n, const double* position, const double* log_scaling, const double* rotation,
                                  const double* alpha_logit, const double* T_camera_world, const double* projection,
                                  int32_t width, int32_t height, double near_plane, double far_plane,
                                  const GsRasterConfigF64* cfg, double* points, double* depth, double* ndc_depth,
                                  int64_t* indexes, int32_t* slot_of, int32_t* num_visible, void* scratch,
                                  int64_t scratch_bytes, void* stream) {
  Args a;
  if (int rc = fill(a, n, position, log_scaling, rotation, alpha_logit, T_camera_world, projection, width, height,
                    near_plane, far_plane, cfg, "gs_project_fwd_f64"))
    return rc;
  GS_REQUIRE(near_plane > 0 && far_plane > near_plane, GS_ERR_INVALID_ARGUMENT, "gs_project_fwd_f64: depth range");
  GS_REQUIRE(num_visible, GS_ERR_INVALID_ARGUMENT, "gs_project_fwd_f64: num_visible is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) {
    if (hipMemsetAsync(num_visible, 0, 4, s) != hipSuccess) {
      gs_set_error("gs_project_fwd_f64: memset failed");
      return GS_ERR_LAUNCH;
    }
    return GS_OK;
  }
  GS_REQUIRE(points && depth && ndc_depth && indexes && slot_of && scratch, GS_ERR_INVALID_ARGUMENT,
             "gs_project_fwd_f64: NULL output");
  GS_REQUIRE(scratch_bytes >= gs_project_f64_scratch_bytes(n), GS_ERR_SCRATCH_TOO_SMALL,
             "gs_project_fwd_f64: scratch %lld < %lld", (long long)scratch_bytes,
             (long long)gs_project_f64_scratch_bytes(n));
  const int nb = int(gs_div_up(n, 256));
  char* p = static_cast<char*>(scratch);
  double* st_rows = reinterpret_cast<double*>(p);
  p += gs_align_up(n * 64, 256);
  int32_t* flags = reinterpret_cast<int32_t*>(p);
  p += gs_align_up(n * 4, 256);
  int32_t* counts = reinterpret_cast<int32_t*>(p);
  p += gs_align_up(int64_t(nb + 1) * 4, 256);
  int32_t* offsets = reinterpret_cast<int32_t*>(p);
  p += gs_align_up(int64_t(nb + 1) * 4, 256);
  hipLaunchKernelGGL(project_f64_kernel, dim3(nb), dim3(256), 0, s, a, st_rows, flags, counts);
  GS_CHECK_LAUNCH("gs_project_fwd_f64/project");
  if (int rc = gs_full_cumsum_i32(nb, counts, offsets, p, gs_cumsum_scratch_bytes(nb), s)) return rc;
  hipLaunchKernelGGL(compact_f64_kernel, dim3(nb), dim3(256), 0, s, n, nb, st_rows, flags, offsets, 1.0 / far_plane,
                     1.0 / near_plane - 1.0 / far_plane, points, depth, ndc_depth, indexes, slot_of, num_visible);
  GS_CHECK_LAUNCH("gs_project_fwd_f64/compact");
  return GS_OK;
}

extern "C" int64_t gs_project_bwd_f64_scratch_bytes(int64_t n) {
  return gs_align_up(gs_div_up(n, 256) * 128, 256) + 256;
}

extern "C" int gs_project_bwd_f64(int64_t n, const double* position, const double* log_scaling, const double* rotation,
                                  const double* alpha_logit, const double* T_camera_world, const double* projection,
                                  int32_t width, int32_t height, const GsRasterConfigF64* cfg, const int32_t* slot_of,
                                  const double* grad_points, const double* grad_depth, double* d_position,
                                  double* d_log_scaling, double* d_rotation, double* d_alpha_logit,
                                  double* d_T_camera_world, double* d_projection, void* scratch,
                                  int64_t scratch_bytes, void* stream) {
  BwdArgs b;
  if (int rc = fill(b.f, n, position, log_scaling, rotation, alpha_logit, T_camera_world, projection, width, height,
                    1.0, 2.0, cfg, "gs_project_bwd_f64"))
    return rc;
  const bool camera = d_T_camera_world != nullptr || d_projection != nullptr;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) {
    if (d_T_camera_world && hipMemsetAsync(d_T_camera_world, 0, 16 * 8, s) != hipSuccess) return GS_ERR_LAUNCH;
    if (d_projection && hipMemsetAsync(d_projection, 0, 4 * 8, s) != hipSuccess) return GS_ERR_LAUNCH;
    return GS_OK;
  }
  GS_REQUIRE(slot_of && d_position && d_log_scaling && d_rotation && d_alpha_logit, GS_ERR_INVALID_ARGUMENT,
             "gs_project_bwd_f64: NULL buffer");
  const int nb = int(gs_div_up(n, 256));
  GS_REQUIRE(!camera || (scratch && scratch_bytes >= gs_project_bwd_f64_scratch_bytes(n)), GS_ERR_SCRATCH_TOO_SMALL,
             "gs_project_bwd_f64: camera gradients need %lld bytes of scratch",
             (long long)gs_project_bwd_f64_scratch_bytes(n));
  b.slot_of = slot_of; b.gpoints = grad_points; b.gdepth = grad_depth;
  b.d_position = d_position; b.d_log_scaling = d_log_scaling; b.d_rotation = d_rotation;
  b.d_alpha_logit = d_alpha_logit;
  b.cam_partials = camera ? static_cast<double*>(scratch) : nullptr;
  hipLaunchKernelGGL(project_bwd_f64_kernel, dim3(nb), dim3(256), 0, s, b);
  GS_CHECK_LAUNCH("gs_project_bwd_f64");
  if (camera) {
    hipLaunchKernelGGL(cam_reduce_f64_kernel, dim3(1), dim3(256), 0, s, nb, b.cam_partials, d_T_camera_world,
                       d_projection);
    GS_CHECK_LAUNCH("gs_project_bwd_f64/camera");
  }
  return GS_OK;
}
