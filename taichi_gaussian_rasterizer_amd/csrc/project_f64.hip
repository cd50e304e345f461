// project_f64.hip -- the perspective projection and its adjoint in float64, for gradcheck.  The per-Gaussian arithmetic
// is the code project.hip compiles -- forward(), visible() and the adjoint row project_bwd_row() of project_math.h --
// instantiated with double (IEEE sqrt / exp / log); the f32 path keeps its own translation unit.  As in f32, a zero
// eigen-gap gives a zero adjoint (DESIGN.md deviation 4).  What is this file's own is what makes the results the same
// bits on every run: a two-pass stable compaction, and camera gradients as per-workgroup partials summed in a fixed
// order.

#include "f64_common.h"
#include "project_math.h"

namespace {

using Args = gs_proj::ProjArgsT<double>;
using Fwd = gs_proj::FwdT<double>;
using BwdArgs = gs_proj::BwdArgsT<double>;

// pass 1: project, stage the row [points(7), depth], count the visible per workgroup
__global__ __launch_bounds__(256) void project_f64_kernel(Args a, double* st_rows, int32_t* flags,
                                                          int32_t* block_counts) {
  __shared__ int32_t s_cnt[4];
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  bool vis = false;
  if (i < a.n) {
    Fwd f;
    gs_proj::forward(a, gs_proj::load_cam(a.T44, a.proj), i, f);
    vis = gs_proj::visible(a, f);
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
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const bool vis = i < n && flags[i] != 0;
  const GsCompactSlot cs = gs_stable_compact<4>(vis, offsets + blockIdx.x, nullptr, 0);
  if (i < n) {
    int slot = -1;
    if (vis) {
      slot = cs.slot;
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

// the adjoint of forward(), one lane per Gaussian (zeros for the culled); CAMERA: plus the workgroup's camera partials
template <bool CAMERA>
__global__ __launch_bounds__(256) void project_bwd_f64_kernel(BwdArgs a) {
  __shared__ double s_red[4];
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  double gcam[16];
  for (int k = 0; k < 16; ++k) gcam[k] = 0.0;
  const int slot = i < a.f.n ? a.slot_of[i] : -1;
  if (i < a.f.n) {
    double dpos[3] = {0, 0, 0}, dls[3] = {0, 0, 0}, dq[4] = {0, 0, 0, 0}, dal = 0;
    if (slot >= 0) gs_proj::project_bwd_row<double, CAMERA>(a, i, slot, dpos, dls, dq, dal, gcam);
    for (int k = 0; k < 3; ++k) a.d_position[3 * i + k] = dpos[k];
    for (int k = 0; k < 3; ++k) a.d_log_scaling[3 * i + k] = dls[k];
    for (int k = 0; k < 4; ++k) a.d_rotation[4 * i + k] = dq[k];
    a.d_alpha_logit[i] = dal;
  }
  if (CAMERA) {
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
  a.inv_far = 1.0 / far_p; a.ndc_denom = 1.0 / near_p - 1.0 / far_p;
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
  hipLaunchKernelGGL(compact_f64_kernel, dim3(nb), dim3(256), 0, s, n, nb, st_rows, flags, offsets, a.inv_far,
                     a.ndc_denom, points, depth, ndc_depth, indexes, slot_of, num_visible);
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
  b.slot_of = slot_of; b.gpoints = grad_points; b.gdepth = grad_depth; b.gdepth_sq = nullptr;
  b.gpoints_stride = 7; b.gdepth_stride = 1;
  b.d_position = d_position; b.d_log_scaling = d_log_scaling; b.d_rotation = d_rotation;
  b.d_alpha_logit = d_alpha_logit;
  b.cam_partials = camera ? static_cast<double*>(scratch) : nullptr;
  if (camera) hipLaunchKernelGGL(project_bwd_f64_kernel<true>, dim3(nb), dim3(256), 0, s, b);
  else hipLaunchKernelGGL(project_bwd_f64_kernel<false>, dim3(nb), dim3(256), 0, s, b);
  GS_CHECK_LAUNCH("gs_project_bwd_f64");
  if (camera) {
    hipLaunchKernelGGL(cam_reduce_f64_kernel, dim3(1), dim3(256), 0, s, nb, b.cam_partials, d_T_camera_world,
                       d_projection);
    GS_CHECK_LAUNCH("gs_project_bwd_f64/camera");
  }
  return GS_OK;
}
