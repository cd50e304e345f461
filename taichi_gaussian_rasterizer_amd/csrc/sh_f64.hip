// sh_f64.hip -- view-dependent colour from real spherical harmonics in float64, and its adjoint, for gradcheck.
// The harmonics and their gradient are the functions sh.hip compiles (sh_math.h, spherical_harmonics.py:38-106),
// instantiated with double; the kernels around them are this file's own (:118-134).  out[c] = clamp(sum_d Y_d(dir) *
// sh[idx,c,d] + 0.5, 0, 1), dir = normalize(p[idx] - camera).
//
// The backward allows repeated indexes without float atomics: the list entries are grouped by Gaussian
// (f64_common.h gs_f64_group) and one lane per Gaussian adds its entries' upstream gradients in ascending list order.
// Every entry of a Gaussian sees the same direction and the same clamp mask, so the lane needs only the sums.

#include "f64_common.h"
#include "sh_math.h"

namespace {

using gs_sh::rsh;
using gs_sh::rsh_grad;

template <int DEG>
__global__ __launch_bounds__(256) void sh_fwd_f64_kernel(int64_t v, int C, const double* params,
                                                         const double* positions, const int64_t* indexes,
                                                         const double* cam, double* out) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= v) return;
  const int64_t idx = indexes[i];
  constexpr int D = (DEG + 1) * (DEG + 1);
  const double dx = positions[3 * idx] - cam[0], dy = positions[3 * idx + 1] - cam[1], dz = positions[3 * idx + 2] - cam[2];
  const double nrm = sqrt(dx * dx + dy * dy + dz * dz);
  double Y[D];
  rsh<double, DEG>(dx / nrm, dy / nrm, dz / nrm, Y);
  for (int c = 0; c < C; ++c) {
    const double* row = params + (idx * C + c) * D;
    double acc = 0.0;
    for (int d = 0; d < D; ++d) acc += Y[d] * row[d];
    const double pre = acc + 0.5;
    out[i * C + c] = pre < 0.0 ? 0.0 : (pre > 1.0 ? 1.0 : pre);  // spherical_harmonics.py:133-134
  }
}

// one lane per Gaussian: its entries order[seg[2 j] .. seg[2 j + 1]) in ascending list order
template <int DEG>
__global__ __launch_bounds__(256) void sh_bwd_f64_kernel(int64_t n, int C, const double* params,
                                                         const double* positions, const int32_t* order,
                                                         const int32_t* seg, const double* cam, const double* gout,
                                                         double* d_params, double* d_positions, double* cam_partials) {
  __shared__ double s_red[4];
  const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
  constexpr int D = (DEG + 1) * (DEG + 1);
  double gd[3] = {0, 0, 0};
  if (j < n) {
    const int e0 = seg[2 * j], e1 = seg[2 * j + 1];
    if (e0 == e1) {
      for (int e = 0; e < C * D; ++e) d_params[j * C * D + e] = 0.0;
    } else {
      const double dx = positions[3 * j] - cam[0], dy = positions[3 * j + 1] - cam[1], dz = positions[3 * j + 2] - cam[2];
      const double nrm = sqrt(dx * dx + dy * dy + dz * dz);
      const double x = dx / nrm, y = dy / nrm, z = dz / nrm;
      double Y[D], w[D];
      rsh<double, DEG>(x, y, z, Y);
      for (int d = 0; d < D; ++d) w[d] = 0.0;
      for (int c = 0; c < C; ++c) {
        const double* row = params + (j * C + c) * D;
        double acc = 0.0;
        for (int d = 0; d < D; ++d) acc += Y[d] * row[d];
        const double pre = acc + 0.5;
        double g = 0.0;
        for (int e = e0; e < e1; ++e) g += gout[int64_t(order[e]) * C + c];
        if (!(pre >= 0.0 && pre <= 1.0)) g = 0.0;  // clamp sub-gradient (1 on the closed interval)
        for (int d = 0; d < D; ++d) {
          d_params[(j * C + c) * D + d] = g * Y[d];
          w[d] += g * row[d];
        }
      }
      if (DEG >= 1) {
        double gdir[3];
        rsh_grad<double, DEG>(x, y, z, w, gdir);
        const double dot = x * gdir[0] + y * gdir[1] + z * gdir[2];
        gd[0] = (gdir[0] - x * dot) / nrm;
        gd[1] = (gdir[1] - y * dot) / nrm;
        gd[2] = (gdir[2] - z * dot) / nrm;
      }
    }
    if (d_positions)
      for (int k = 0; k < 3; ++k) d_positions[3 * j + k] = gd[k];
  }
  if (cam_partials)
    for (int k = 0; k < 3; ++k) {
      const double t = gs_f64_block_sum<4>(gd[k], s_red);
      if (threadIdx.x == 0) cam_partials[int64_t(blockIdx.x) * 3 + k] = t;
    }
}

// d_camera_pos = -(sum of the workgroups' partials), in a fixed order
__global__ __launch_bounds__(256) void sh_cam_reduce_f64_kernel(int num_blocks, const double* partials, double* d_cam) {
  __shared__ double s_red[4];
  for (int k = 0; k < 3; ++k) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < num_blocks; b += 256) acc += partials[int64_t(b) * 3 + k];
    const double t = gs_f64_block_sum<4>(acc, s_red);
    if (threadIdx.x == 0) d_cam[k] = -t;
  }
}

int check_sh(int64_t n, int64_t v, int32_t C, int32_t degree, const char* what) {
  GS_REQUIRE(degree >= 0 && degree <= 3, GS_ERR_UNSUPPORTED, "%s: SH degree %d (0 to 3)", what, degree);
  GS_REQUIRE(C >= 1 && C <= GS_MAX_SH_CHANNELS, GS_ERR_UNSUPPORTED, "%s: %d channels (1 to %d)", what, C,
             GS_MAX_SH_CHANNELS);
  GS_REQUIRE(n >= 0 && n < (int64_t(1) << 31) && v >= 0 && v < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT,
             "%s: %lld gaussians, %lld indexes", what, (long long)n, (long long)v);
  return GS_OK;
}

}  // namespace

extern "C" int gs_sh_fwd_f64(int64_t v, int32_t channels, int32_t degree, const double* params,
                             const double* positions, const int64_t* indexes, const double* camera_pos, double* out,
                             void* stream) {
  if (int rc = check_sh(0, v, channels, degree, "gs_sh_fwd_f64")) return rc;
  if (v == 0) return GS_OK;
  GS_REQUIRE(params && positions && indexes && camera_pos && out, GS_ERR_INVALID_ARGUMENT, "gs_sh_fwd_f64: NULL buffer");
#define SH_FWD_F64(DEG)                                                                                              \
  hipLaunchKernelGGL(sh_fwd_f64_kernel<DEG>, dim3(gs_div_up(v, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), \
                     v, channels, params, positions, indexes, camera_pos, out)
  switch (degree) {
    case 0: SH_FWD_F64(0); break;
    case 1: SH_FWD_F64(1); break;
    case 2: SH_FWD_F64(2); break;
    default: SH_FWD_F64(3); break;
  }
  GS_CHECK_LAUNCH("gs_sh_fwd_f64");
  return GS_OK;
}

extern "C" int64_t gs_sh_bwd_f64_scratch_bytes(int64_t n, int64_t v) {
  return gs_align_up(gs_div_up(n, 256) * 24 + 8, 256) + gs_f64_group_scratch_bytes(v, n, 8);
}

extern "C" int gs_sh_bwd_f64(int64_t n, int64_t v, int32_t channels, int32_t degree, const double* params,
                             const double* positions, const int64_t* indexes, const double* camera_pos,
                             const double* grad_out, double* d_params, double* d_positions, double* d_camera_pos,
                             void* scratch, int64_t scratch_bytes, void* stream) {
  if (int rc = check_sh(n, v, channels, degree, "gs_sh_bwd_f64")) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) {
    if (d_camera_pos && hipMemsetAsync(d_camera_pos, 0, 3 * 8, s) != hipSuccess) return GS_ERR_LAUNCH;
    return GS_OK;
  }
  GS_REQUIRE(params && positions && camera_pos && d_params && (v == 0 || (indexes && grad_out)),
             GS_ERR_INVALID_ARGUMENT, "gs_sh_bwd_f64: NULL buffer");
  GS_REQUIRE(scratch && scratch_bytes >= gs_sh_bwd_f64_scratch_bytes(n, v), GS_ERR_SCRATCH_TOO_SMALL,
             "gs_sh_bwd_f64: scratch %lld < %lld", (long long)scratch_bytes,
             (long long)gs_sh_bwd_f64_scratch_bytes(n, v));
  const int nb = int(gs_div_up(n, 256));
  double* partials = static_cast<double*>(scratch);
  const int64_t pb = gs_align_up(int64_t(nb) * 24 + 8, 256);
  int32_t *order, *seg;
  if (int rc = gs_f64_group(v, 8, indexes, n, &order, &seg, static_cast<char*>(scratch) + pb, scratch_bytes - pb, s))
    return rc;
#define SH_BWD_F64(DEG)                                                                                             \
  hipLaunchKernelGGL(sh_bwd_f64_kernel<DEG>, dim3(nb), dim3(256), 0, s, n, channels, params, positions, order, seg, \
                     camera_pos, grad_out, d_params, d_positions, d_camera_pos ? partials : nullptr)
  switch (degree) {
    case 0: SH_BWD_F64(0); break;
    case 1: SH_BWD_F64(1); break;
    case 2: SH_BWD_F64(2); break;
    default: SH_BWD_F64(3); break;
  }
  GS_CHECK_LAUNCH("gs_sh_bwd_f64");
  if (d_camera_pos) {
    hipLaunchKernelGGL(sh_cam_reduce_f64_kernel, dim3(1), dim3(256), 0, s, nb, partials, d_camera_pos);
    GS_CHECK_LAUNCH("gs_sh_bwd_f64/camera");
  }
  return GS_OK;
}
