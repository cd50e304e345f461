// project.hip -- perspective projection + EWA 3D->2D covariance + cull + compaction, and its
// hand-derived adjoint.  Reference: perspective/projection.py:32-80 (project_kernel), :84-118
// (indexed_project_kernel, differentiated by Taichi autodiff at :175-180), math in
// taichi_lib/generic.py:96-158, :217-237, :419-427; ndc depth torch_lib/projection.py:120-123.
//
// MI355X notes: one lane per Gaussian, inputs read once (44 B/Gaussian); the camera (16+4 floats)
// is read through wave-uniform scalar loads instead of the reference's per-point expanded copies
// (projection.py:212-213: +64 B/Gaussian).  Compaction (the reference's torch.nonzero + two
// gathers, :146-149) is a ballot/popcount rank inside each 256-lane block plus one scan of the
// per-block counts; ndc depth and the int64 index list come out of the same pass.
//
// Roofline (HBM): forward reads 44 N, writes 36 N staging + reads it back + 48 V out;
// backward reads 44 N + 36 V, writes 44 N.

#include "gs_common.h"
#include "../../include/gs_detmath.h"
#include "project_math.h"

namespace {

using namespace gs_proj;

// pass 1: project everything, stage rows, count visible per block
// zero_words: the tile mapper's region counters, which the compaction pass adds into when it also does the mapper's
// binning (frame calls): cleared here, one pass earlier, instead of by a memset launch
__global__ __launch_bounds__(256) void project_kernel(ProjArgs a, float4* st_rows, int* block_counts, float* cam_out,
                                                      int* zero_words, int zero_count) {
  __shared__ int s_cnt[4];
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (cam_out && blockIdx.x == 0 && threadIdx.x == 0) camera_position(a.T44, cam_out);
  if (zero_words && blockIdx.x == 0)
    for (int e = threadIdx.x; e < zero_count; e += 256) zero_words[e] = 0;
  bool vis = false;
  if (i < a.n) {
    const Cam c = load_cam(a.T44, a.proj);
    Fwd f;
    forward(a, c, i, f);
    vis = visible(a, f);
    const float z = f.cam[2];
    st_rows[2 * i] = make_float4(f.u, f.v, f.ax, f.ay);
    st_rows[2 * i + 1] = make_float4(f.s1, f.s2, f.alpha, vis ? z : 0.0f);  // depth 0 = culled (:69-70)
  }
  const uint64_t b = __ballot(vis);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// pass 2: stable compaction
// block_offsets == nullptr: every workgroup sums the visible counts of the workgroups before it itself
// (block_counts, a few KB that stay in L2) instead of reading a prefix computed by three scan launches
__global__ __launch_bounds__(256) void compact_kernel(GsCompactArgs c) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const float4* st_rows = static_cast<const float4*>(c.st_rows);
  float4 r0 = make_float4(0, 0, 0, 0), r1 = r0;
  bool vis = false;
  if (i < c.n) {
    r0 = st_rows[2 * i];
    r1 = st_rows[2 * i + 1];
    vis = r1.w != 0.0f;
  }
  const GsCompactSlot k = gs_stable_compact<4>(vis, c.block_offsets ? c.block_offsets + blockIdx.x : nullptr,
                                               c.block_counts, int(blockIdx.x));
  if (i < c.n) {
    if (vis) gs_write_compact_row(c, k.slot, i, r0, r1);
    c.slot_of[i] = vis ? k.slot : -1;
  }
  // the frame's gradient rows (gs_raster_bwd accumulates into them with atomics): zero-filled here, by the pass that
  // already streams the V compact rows, instead of by a fill launch in front of the backward.  The workgroup's rows are
  // one contiguous range, cleared with consecutive 16-byte stores (a lane clearing its own 64-byte row costs 12 us more)
  if (c.zero_rows) {
    float4* dst = static_cast<float4*>(c.zero_rows) + int64_t(k.first) * c.zero_row_v4;
    for (int e = threadIdx.x; e < k.total * c.zero_row_v4; e += 256) dst[e] = make_float4(0, 0, 0, 0);
  }
  if (int(blockIdx.x) == c.num_blocks - 1 && threadIdx.x == 0) *c.num_visible = k.first + k.total;
}

// ------------------------------------------------------------------------------- backward
// (BwdArgs and the adjoint of one visible Gaussian, project_bwd_row: project_math.h)

// One lane of the adjoint, whole: Gaussian i (if `valid`), upstream gradients in row `slot` (< 0: culled, zeros), the
// four gradients to row `out`; then the block's camera partials.  The dense and the row-compact kernel differ only in
// how they find (i, slot, out) -- everything that computes is this one body, under the same control flow.
template <bool CAMERA>
__device__ __forceinline__ void project_bwd_lane(const BwdArgs& a, const bool valid, const int64_t i, const int slot,
                                                 const int64_t out) {
  float gcam_acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) gcam_acc[k] = 0.0f;
  if (valid) {
    float dpos[3] = {0, 0, 0}, dls[3] = {0, 0, 0}, dq[4] = {0, 0, 0, 0}, dal = 0;
    if (slot >= 0) {
      project_bwd_row<float, CAMERA>(a, i, slot, dpos, dls, dq, dal, gcam_acc);
    }
#pragma unroll
    // gradients are written once and read by the optimizer later: keep them out of the caches the next frame's
    // gathers live in
    for (int k = 0; k < 3; ++k) __builtin_nontemporal_store(dpos[k], a.d_position + 3 * out + k);
#pragma unroll
    for (int k = 0; k < 3; ++k) __builtin_nontemporal_store(dls[k], a.d_log_scaling + 3 * out + k);
#pragma unroll
    for (int k = 0; k < 4; ++k) __builtin_nontemporal_store(dq[k], a.d_rotation + 4 * out + k);
    __builtin_nontemporal_store(dal, a.d_alpha_logit + out);
  }
  if (CAMERA) {
    __shared__ float s_part[4][16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float tot = gs_wave_sum_to_lane63(gcam_acc[k]);
      if ((threadIdx.x & 63) == 63) s_part[threadIdx.x >> 6][k] = tot;
    }
    __syncthreads();
    if (threadIdx.x < 16)
      a.cam_partials[int64_t(blockIdx.x) * 16 + threadIdx.x] =
          s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
  }
}

template <bool CAMERA>
__global__ __launch_bounds__(256) void project_bwd_kernel(BwdArgs a) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const int slot = i < a.f.n ? a.slot_of[i] : -1;
  project_bwd_lane<CAMERA>(a, i < a.f.n, i, slot, i);
}

// Row-compact variant: one lane per VISIBLE row r (Gaussian indexes[r], the upstream gradient is row r), the four
// gradients go to row r of (v, 3) (v, 3) (v, 4) (v, 1) arrays -- nothing is written for the culled Gaussians.  The camera
// partials are per block of visible rows.  (A negative index, which the visible list never holds, would be a culled row:
// the test keeps the control flow of the shared body that of the dense kernel.)
template <bool CAMERA>
__global__ __launch_bounds__(256) void project_bwd_rows_kernel(BwdArgs a, const int64_t* indexes, int64_t v) {
  const int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const int64_t i = r < v ? indexes[r] : -1;
  project_bwd_lane<CAMERA>(a, r < v, i, i >= 0 ? int(r) : -1, r);
}

// deterministic final reduction of the per-block camera partials (one block, fixed order)
__global__ __launch_bounds__(256) void cam_reduce_kernel(int num_blocks, const float* partials, float* dT44, float* dproj) {
  __shared__ double s[256];
  for (int k = 0; k < 16; ++k) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < num_blocks; b += 256) acc += double(partials[int64_t(b) * 16 + k]);
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      if (k < 12) { if (dT44) dT44[k] = float(s[0]); }
      else if (dproj) dproj[k - 12] = float(s[0]);
    }
    __syncthreads();
  }
  if (threadIdx.x < 4 && dT44) dT44[12 + threadIdx.x] = 0.0f;
}

__global__ void camera_position_kernel(const float* T, float* out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) camera_position(T, out);
}

int fill(ProjArgs& a, int64_t n, const float* position, const float* log_scaling, const float* rotation,
         const float* alpha_logit, const float* T, const float* proj, int width, int height, double near_p,
         double far_p, const GsRasterConfig* cfg) {
  if (int rc = gs_check_cfg(cfg)) return rc;
  GS_REQUIRE(n >= 0 && n < (int64_t(1) << 31), GS_ERR_INVALID_ARGUMENT, "projection: %lld gaussians", (long long)n);
  GS_REQUIRE(width > 0 && height > 0, GS_ERR_INVALID_ARGUMENT, "projection: image size %dx%d", width, height);
  GS_REQUIRE(n == 0 || (position && log_scaling && rotation && alpha_logit), GS_ERR_INVALID_ARGUMENT,
             "projection: NULL gaussian tensor");
  GS_REQUIRE(T && proj, GS_ERR_INVALID_ARGUMENT, "projection: NULL camera");
  a.position = position; a.log_scaling = log_scaling; a.rotation = rotation; a.alpha_logit = alpha_logit;
  a.T44 = T; a.proj = proj; a.n = n;
  a.width = float(width); a.height = float(height);
  a.near_p = float(near_p); a.far_p = float(far_p);
  a.inv_far = float(1.0 / far_p);
  a.ndc_denom = float(1.0 / near_p - 1.0 / far_p);
  a.clamp_margin = cfg->clamp_margin; a.blur_cov = cfg->blur_cov; a.alpha_thr = cfg->alpha_threshold;
  return GS_OK;
}

}  // namespace

extern "C" int64_t gs_project_scratch_bytes(int64_t n) {
  const int64_t nb = gs_div_up(n, 256);
  return gs_align_up(n * 32, 256) + gs_align_up((nb + 1) * 4, 256) * 2 + gs_cumsum_scratch_bytes(nb) + 256;
}

extern "C" int gs_project_fwd(int64_t n, const float* position, const float* log_scaling, const float* rotation,
                              const float* alpha_logit, const float* T_camera_world, const float* projection,
                              int32_t width, int32_t height, double near_plane, double far_plane,
                              const GsRasterConfig* cfg, float* points, float* depth, float* ndc_depth,
                              int64_t* indexes, int32_t* slot_of, int32_t* num_visible, float* depth_features,
                              int32_t depth_features_stride, float* camera_pos, void* scratch,
                              int64_t scratch_bytes, void* stream) {
  return gs_project_fwd_ex(n, position, log_scaling, rotation, alpha_logit, T_camera_world, projection, width, height,
                           near_plane, far_plane, cfg, points, depth, ndc_depth, indexes, slot_of, num_visible,
                           depth_features, depth_features_stride, camera_pos, scratch, scratch_bytes, nullptr, 0, nullptr,
                           stream);
}

// gs_project_fwd + (library-internal, used by gs_frame_fwd) zero_rows: a (V, zero_row_floats) buffer, 16-byte aligned
// rows, whose first V rows the compaction pass zero-fills; bin: the compaction pass also does the tile mapper's region
// binning (gs_common.h: GsMapBinPlan)
int gs_project_fwd_ex(int64_t n, const float* position, const float* log_scaling, const float* rotation,
                      const float* alpha_logit, const float* T_camera_world, const float* projection, int32_t width,
                      int32_t height, double near_plane, double far_plane, const GsRasterConfig* cfg, float* points,
                      float* depth, float* ndc_depth, int64_t* indexes, int32_t* slot_of, int32_t* num_visible,
                      float* depth_features, int32_t depth_features_stride, float* camera_pos, void* scratch,
                      int64_t scratch_bytes, float* zero_rows, int32_t zero_row_floats, const GsMapBinPlan* bin,
                      void* stream) {
  ProjArgs a;
  if (int rc = fill(a, n, position, log_scaling, rotation, alpha_logit, T_camera_world, projection, width, height,
                    near_plane, far_plane, cfg))
    return rc;
  GS_REQUIRE(near_plane > 0 && far_plane > near_plane, GS_ERR_INVALID_ARGUMENT, "projection: depth range");
  GS_REQUIRE(num_visible, GS_ERR_INVALID_ARGUMENT, "gs_project_fwd: num_visible is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) {
    if (hipMemsetAsync(num_visible, 0, 4, s) != hipSuccess) { gs_set_error("gs_project_fwd: memset failed"); return GS_ERR_LAUNCH; }
    if (camera_pos) return gs_camera_position(T_camera_world, camera_pos, stream);
    return GS_OK;
  }
  GS_REQUIRE(points && depth && ndc_depth && indexes && slot_of && scratch, GS_ERR_INVALID_ARGUMENT,
             "gs_project_fwd: NULL output");
  GS_REQUIRE(scratch_bytes >= gs_project_scratch_bytes(n), GS_ERR_SCRATCH_TOO_SMALL,
             "gs_project_fwd: scratch %lld < %lld", (long long)scratch_bytes, (long long)gs_project_scratch_bytes(n));
  const int nb = int(gs_div_up(n, 256));
  char* base = static_cast<char*>(scratch);
  float4* st_rows = reinterpret_cast<float4*>(base);
  int* counts = reinterpret_cast<int*>(base + gs_align_up(n * 32, 256));
  int* offsets = counts + gs_align_up(int64_t(nb + 1) * 4, 256) / 4;
  void* scan_scratch = offsets + gs_align_up(int64_t(nb + 1) * 4, 256) / 4;
  int32_t* zero_words = nullptr;
  int32_t zero_count = 0;
  if (bin)
    if (int rc = gs_map_bin_counters(bin, n, &zero_words, &zero_count)) return rc;
  hipLaunchKernelGGL(project_kernel, dim3(nb), dim3(256), 0, s, a, st_rows, counts, camera_pos, zero_words, zero_count);
  GS_CHECK_LAUNCH("gs_project_fwd/project");
  // up to 16384 workgroups (4M Gaussians) each workgroup adds up the counts in front of it (<= 64 KB out of
  // L2); beyond that the quadratic read volume loses to a proper scan
  const bool self_offsets = nb <= 16384;
  if (!self_offsets)
    if (int rc = gs_full_cumsum_i32(nb, counts, offsets, scan_scratch, gs_cumsum_scratch_bytes(nb), s)) return rc;
  GsCompactArgs c;
  c.n = n; c.st_rows = st_rows; c.block_offsets = self_offsets ? nullptr : offsets; c.block_counts = counts;
  c.num_blocks = nb; c.inv_far = a.inv_far; c.ndc_denom = a.ndc_denom;
  c.points = points; c.depth = depth; c.ndc = ndc_depth; c.indexes = indexes; c.slot_of = slot_of;
  c.num_visible = num_visible; c.depth_feat = depth_features; c.depth_feat_stride = depth_features_stride;
  c.zero_rows = zero_rows; c.zero_row_v4 = zero_row_floats / 4;
  if (bin) return gs_map_compact_bin(bin, &c, stream);
  hipLaunchKernelGGL(compact_kernel, dim3(nb), dim3(256), 0, s, c);
  GS_CHECK_LAUNCH("gs_project_fwd/compact");
  return GS_OK;
}

extern "C" int64_t gs_project_bwd_scratch_bytes(int64_t n) { return gs_align_up(gs_div_up(n, 256) * 64, 256) + 256; }

extern "C" int gs_project_bwd(int64_t n, int64_t v, const float* position, const float* log_scaling,
                              const float* rotation, const float* alpha_logit, const float* T_camera_world,
                              const float* projection, int32_t width, int32_t height, const GsRasterConfig* cfg,
                              const int32_t* slot_of, const float* grad_points, int32_t grad_points_stride,
                              const float* grad_depth, const float* grad_depth_sq, int32_t grad_depth_stride,
                              float* d_position, float* d_log_scaling, float* d_rotation, float* d_alpha_logit,
                              float* d_T_camera_world, float* d_projection, void* scratch, int64_t scratch_bytes,
                              void* stream) {
  (void)v;
  BwdArgs b;
  if (int rc = fill(b.f, n, position, log_scaling, rotation, alpha_logit, T_camera_world, projection, width, height,
                    1.0, 2.0, cfg))
    return rc;
  if (n == 0) return GS_OK;
  GS_REQUIRE(slot_of && d_position && d_log_scaling && d_rotation && d_alpha_logit, GS_ERR_INVALID_ARGUMENT,
             "gs_project_bwd: NULL buffer");
  const bool camera = d_T_camera_world != nullptr || d_projection != nullptr;
  const int nb = int(gs_div_up(n, 256));
  GS_REQUIRE(!camera || (scratch && scratch_bytes >= int64_t(nb) * 64), GS_ERR_SCRATCH_TOO_SMALL,
             "gs_project_bwd: camera gradients need %lld bytes of scratch", (long long)(int64_t(nb) * 64));
  b.slot_of = slot_of; b.gpoints = grad_points; b.gdepth = grad_depth; b.gdepth_sq = grad_depth_sq;
  b.gpoints_stride = grad_points_stride > 0 ? grad_points_stride : 7;
  b.gdepth_stride = grad_depth_stride > 0 ? grad_depth_stride : 1;
  b.d_position = d_position; b.d_log_scaling = d_log_scaling; b.d_rotation = d_rotation;
  b.d_alpha_logit = d_alpha_logit;
  b.cam_partials = static_cast<float*>(scratch);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (camera) {
    hipLaunchKernelGGL(project_bwd_kernel<true>, dim3(nb), dim3(256), 0, s, b);
    hipLaunchKernelGGL(cam_reduce_kernel, dim3(1), dim3(256), 0, s, nb, b.cam_partials, d_T_camera_world,
                       d_projection);
  } else {
    hipLaunchKernelGGL(project_bwd_kernel<false>, dim3(nb), dim3(256), 0, s, b);
  }
  GS_CHECK_LAUNCH("gs_project_bwd");
  return GS_OK;
}

extern "C" int64_t gs_project_bwd_rows_scratch_bytes(int64_t v) { return gs_project_bwd_scratch_bytes(v); }

extern "C" int gs_project_bwd_rows(int64_t n, int64_t v, const float* position, const float* log_scaling,
                                   const float* rotation, const float* alpha_logit, const float* T_camera_world,
                                   const float* projection, int32_t width, int32_t height, const GsRasterConfig* cfg,
                                   const int64_t* indexes, const float* grad_points, int32_t grad_points_stride,
                                   const float* grad_depth, const float* grad_depth_sq, int32_t grad_depth_stride,
                                   float* d_position, float* d_log_scaling, float* d_rotation, float* d_alpha_logit,
                                   float* d_T_camera_world, float* d_projection, void* scratch, int64_t scratch_bytes,
                                   void* stream) {
  BwdArgs b;
  if (int rc = fill(b.f, n, position, log_scaling, rotation, alpha_logit, T_camera_world, projection, width, height,
                    1.0, 2.0, cfg))
    return rc;
  GS_REQUIRE(v >= 0 && v <= n, GS_ERR_INVALID_ARGUMENT, "gs_project_bwd_rows: %lld visible rows of %lld gaussians",
             (long long)v, (long long)n);
  const bool camera = d_T_camera_world != nullptr || d_projection != nullptr;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (v == 0) {
    // nothing is visible: the camera gradients are the empty sum
    bool ok = true;
    if (d_T_camera_world) ok &= hipMemsetAsync(d_T_camera_world, 0, 64, s) == hipSuccess;
    if (d_projection) ok &= hipMemsetAsync(d_projection, 0, 16, s) == hipSuccess;
    if (!ok) { gs_set_error("gs_project_bwd_rows: hipMemsetAsync failed"); return GS_ERR_LAUNCH; }
    return GS_OK;
  }
  GS_REQUIRE(indexes && d_position && d_log_scaling && d_rotation && d_alpha_logit, GS_ERR_INVALID_ARGUMENT,
             "gs_project_bwd_rows: NULL buffer");
  const int nb = int(gs_div_up(v, 256));
  GS_REQUIRE(!camera || (scratch && scratch_bytes >= int64_t(nb) * 64), GS_ERR_SCRATCH_TOO_SMALL,
             "gs_project_bwd_rows: camera gradients need %lld bytes of scratch", (long long)(int64_t(nb) * 64));
  b.slot_of = nullptr; b.gpoints = grad_points; b.gdepth = grad_depth; b.gdepth_sq = grad_depth_sq;
  b.gpoints_stride = grad_points_stride > 0 ? grad_points_stride : 7;
  b.gdepth_stride = grad_depth_stride > 0 ? grad_depth_stride : 1;
  b.d_position = d_position; b.d_log_scaling = d_log_scaling; b.d_rotation = d_rotation;
  b.d_alpha_logit = d_alpha_logit;
  b.cam_partials = static_cast<float*>(scratch);
  if (camera) {
    hipLaunchKernelGGL(project_bwd_rows_kernel<true>, dim3(nb), dim3(256), 0, s, b, indexes, v);
    hipLaunchKernelGGL(cam_reduce_kernel, dim3(1), dim3(256), 0, s, nb, b.cam_partials, d_T_camera_world,
                       d_projection);
  } else {
    hipLaunchKernelGGL(project_bwd_rows_kernel<false>, dim3(nb), dim3(256), 0, s, b, indexes, v);
  }
  GS_CHECK_LAUNCH("gs_project_bwd_rows");
  return GS_OK;
}

extern "C" int gs_camera_position(const float* T_camera_world, float* camera_pos, void* stream) {
  GS_REQUIRE(T_camera_world && camera_pos, GS_ERR_INVALID_ARGUMENT, "gs_camera_position: NULL buffer");
  hipLaunchKernelGGL(camera_position_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), T_camera_world,
                     camera_pos);
  GS_CHECK_LAUNCH("gs_camera_position");
  return GS_OK;
}
