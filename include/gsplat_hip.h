/* gsplat_hip.h -- C-ABI of libgsplat_hip.so: the MI355X (gfx950) render path behind the
 * taichi_splatting operator API.
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - every pointer is a caller-owned DEVICE buffer unless the name ends in _host; nothing is
 *     allocated or freed inside the library; scratch comes from the caller (sizes below).
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     all work is enqueued on it and no entry point synchronises the device.  Host-visible
 *     counts (V, K) are written to device int32 words that the caller reads back itself.
 *   - return value: 0 on success, negative GsStatus on failure; gs_last_error() returns a
 *     thread-local message for the last failure on the calling thread.
 *   - re-entrant, no global mutable state.
 *   - f32, except the gs_*_f64 entry points at the end: float64 projection, SH and rasterizer for
 *     gradcheck (the reference's f64 instantiations, taichi_lib/__init__.py:8-14).
 *
 * "replaces" lines cite the reference interface each entry point stands in for (paths relative
 * to /root/reference/taichi_splatting/).  The reference-side binding is in INTEGRATION.md.
 */
#ifndef GSPLAT_HIP_H
#define GSPLAT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum GsStatus {
  GS_OK = 0,
  GS_ERR_INVALID_ARGUMENT = -1,
  GS_ERR_UNSUPPORTED = -2,   /* e.g. tile_size not in {8,16,32}, feature width > GS_MAX_FEATURES */
  GS_ERR_LAUNCH = -3,        /* hipGetLastError() after a launch */
  GS_ERR_SCRATCH_TOO_SMALL = -4
} GsStatus;

#define GS_MAX_FEATURES 32
#define GS_MAX_WIDE_FEATURES 512 /* gs_raster_fwd_wide / gs_raster_bwd_wide */
#define GS_MAX_SH_CHANNELS 8

/* Mirrors RasterConfig (data_types.py:13-39) field for field. */
typedef struct GsRasterConfig {
  int32_t tile_size;            /* 8, 16 or 32 */
  int32_t pixel_stride_x;       /* accepted, ignored: thread<->pixel mapping only (rasterizer/tiling.py:35-65) */
  int32_t pixel_stride_y;
  int32_t antialias;
  int32_t use_alpha_blending;
  int32_t compute_point_heuristic;
  int32_t compute_visibility;
  float clamp_margin;
  float blur_cov;
  float clamp_max_alpha;
  float alpha_threshold;
  float saturate_threshold;
  /* Not a reference field.  The reference's forward keeps blending down a tile's whole list (forward.py:84-128);
   * this library stops a 16x16 region once EVERY pixel of it has less than forward_cut of its transmittance left.
   * What is dropped changes a pixel by less than forward_cut * max|feature|.  0 is the setting closest to the
   * reference: values below 2^-25 act as 2^-25, half an ulp of 1, below which the reference's own f32 accumulation
   * W += w no longer changes W (this library carries the transmittance T = 1 - W itself, which would keep
   * shrinking); the reference still adds alpha * (1 - W) * feature there with 1 - W stuck at ~2^-24, so the two differ
   * by less than N * 2^-24 * max|feature| for N remaining splats (no reference fixture pins this).
   * The Python layer passes RasterConfig.forward_cut (default 2^-20), divided by the squared far plane when the
   * z / z^2 depth features are blended, so the bound is relative to the feature magnitude. */
  float forward_cut;
  /* Developer tuning aids, per call (the library reads no environment variable and keeps no global state); results
   * never depend on them.  tune_wave_sub_blocks: 0 = choose the rasterizer's wave region from the grid size, 1 | 2 | 4
   * = force 8x8 / 16x8 / 16x16 pixels per wave.  tune_no_heavy_split: 1 = never give the fullest tiles four
   * workgroups. */
  int32_t tune_wave_sub_blocks;
  int32_t tune_no_heavy_split;
} GsRasterConfig;

/* Screen-tile sharding (the reference has no counterpart): which tile ROWS of the full image one call
 * covers.  Row ty is owned iff row_begin <= ty < row_end and (period <= 1 or (ty / band) % period == phase);
 * owned rows keep their order and are numbered 0, 1, ... ("local rows").  period <= 1: one contiguous strip;
 * period > 1 (with row_begin = 0, row_end = all rows): bands of `band` rows dealt round-robin to `period` owners
 * (interleaved strips, load balance on real scenes).  With a shard, `height` stays the FULL image height, splat
 * coordinates stay full-image coordinates, tile ids / tile_ranges / tile_order are local (local row * tiles_wide +
 * column) and image buffers hold the owned pixel rows only, in order.  NULL = the whole image. */
typedef struct GsRowShard {
  int32_t row_begin, row_end;
  int32_t band, period, phase;
} GsRowShard;

const char* gs_last_error(void);
int gs_version(void);

/* ------------------------------------------------------------------ projection (a2, a3) --
 * replaces: perspective/projection.py:32-80 project_kernel + :146-149 (nonzero + gathers) and
 * torch_lib/projection.py:120-123 ndc_depth (called renderer.py:189).
 *
 * Step 1 projects all n Gaussians into n-row staging buffers and counts the visible ones per
 * 256-thread block; step 2 scans the block counts and compacts, in ascending index order, into
 * buffers the caller sized for n rows (only the first V rows are written).  *num_visible
 * (device int32) receives V.
 *   T_camera_world: 16 floats row-major 4x4 (device), projection: [fx,fy,cx,cy] (device).
 *   points: (V,7) [mean.xy, axis.xy, sigma.xy, alpha]; depth: (V) camera z; ndc_depth: (V)
 *   = 1 - (1/z - (float)(1/far)) / (float)(1/near - 1/far)  (fixed f32 op order);
 *   indexes: (V) int64 ascending; slot_of: (n) int32, compact row of Gaussian i or -1.
 *   depth_features (optional): row i of a (V, depth_features_stride) raster-feature buffer receives
 *   [z, z^2] in its first two columns (renderer.py:191-193, render_depth=True).
 *   camera_pos (optional, 3 floats): receives the camera centre, as gs_camera_position would (saves its launch).
 * scratch: gs_project_scratch_bytes(n).
 */
int64_t gs_project_scratch_bytes(int64_t n);
int gs_project_fwd(int64_t n, const float* position, const float* log_scaling, const float* rotation,
                   const float* alpha_logit, const float* T_camera_world, const float* projection, int32_t width,
                   int32_t height, double near_plane, double far_plane, const GsRasterConfig* cfg, float* points,
                   float* depth, float* ndc_depth, int64_t* indexes, int32_t* slot_of, int32_t* num_visible,
                   float* depth_features, int32_t depth_features_stride, float* camera_pos,
                   void* scratch, int64_t scratch_bytes, void* stream);

/* replaces: perspective/projection.py:84-118 indexed_project_kernel.grad (Taichi autodiff,
 * :166-185).  Hand-derived adjoint.  Dense gradients (rows of culled Gaussians are zero);
 * d_T_camera_world is 16 floats (last row zero) and d_projection 4 floats, summed over the
 * visible set (the reference sums its per-point expanded copies, :212-213).  Either may be NULL.
 * grad_points (row stride grad_points_stride, <= 0 means 7), grad_depth and grad_depth_sq (stride
 * grad_depth_stride, <= 0 means 1) may be NULL (treated as zero); grad_depth_sq is the gradient of a
 * z^2 feature and contributes 2 z g (so the rasterizer's gradient rows can be consumed in place).
 * scratch: gs_project_bwd_scratch_bytes(n) (per-block camera partials; unused when both camera
 * outputs are NULL).
 */
int64_t gs_project_bwd_scratch_bytes(int64_t n);
int gs_project_bwd(int64_t n, int64_t v, const float* position, const float* log_scaling, const float* rotation,
                   const float* alpha_logit, const float* T_camera_world, const float* projection, int32_t width,
                   int32_t height, const GsRasterConfig* cfg, const int32_t* slot_of, const float* grad_points,
                   int32_t grad_points_stride, const float* grad_depth, const float* grad_depth_sq,
                   int32_t grad_depth_stride, float* d_position, float* d_log_scaling, float* d_rotation,
                   float* d_alpha_logit, float* d_T_camera_world, float* d_projection, void* scratch,
                   int64_t scratch_bytes, void* stream);

/* Row-compact projection adjoint (no reference counterpart: sparse visible-row gradients): gs_project_bwd for the v
 * visible rows only.  indexes (v) int64: the visible list of gs_project_fwd (ascending, distinct); the upstream
 * gradients are read at row i (same striding rules), the four gradients are written to ROW i of d_position (v,3),
 * d_log_scaling (v,3), d_rotation (v,4), d_alpha_logit (v,1) -- nothing is written for the culled Gaussians, and row i
 * holds the bits gs_project_bwd writes to row indexes[i].  d_T_camera_world / d_projection as in gs_project_bwd
 * (per-block partials of the visible rows, summed in a fixed order; zeros for v == 0).
 * scratch: gs_project_bwd_rows_scratch_bytes(v), unused when both camera outputs are NULL. */
int64_t gs_project_bwd_rows_scratch_bytes(int64_t v);
int gs_project_bwd_rows(int64_t n, int64_t v, const float* position, const float* log_scaling, const float* rotation,
                        const float* alpha_logit, const float* T_camera_world, const float* projection, int32_t width,
                        int32_t height, const GsRasterConfig* cfg, const int64_t* indexes, const float* grad_points,
                        int32_t grad_points_stride, const float* grad_depth, const float* grad_depth_sq,
                        int32_t grad_depth_stride, float* d_position, float* d_log_scaling, float* d_rotation,
                        float* d_alpha_logit, float* d_T_camera_world, float* d_projection, void* scratch,
                        int64_t scratch_bytes, void* stream);

/* replaces: CameraParams.camera_position (perspective/params.py:76-78, torch.inverse(T)[0:3,3]) for an
 * affine camera matrix (last row 0 0 0 1), computed on the device without a host round trip. */
int gs_camera_position(const float* T_camera_world, float* camera_pos, void* stream);

/* ------------------------------------------------------------ spherical harmonics (a4) --
 * replaces: spherical_harmonics.py:118-134 evaluate_sh_at_kernel (+ .grad, :154-161).
 * params (n,C,D) D=(degree+1)^2, degree 0..3, C <= GS_MAX_SH_CHANNELS; positions (n,3);
 * indexes (v) int64 (may repeat); camera_pos 3 floats (device); out (v,C), row stride out_stride
 * (<= 0 means C).  v_dev (optional, device int32): the live row count when v is only a capacity.
 * Backward: d_params (n,C,D) and d_positions (n,3) are zero-filled inside, then written.  When
 * indexes_unique != 0 (the list came from gs_project_fwd) rows are written with plain stores;
 * otherwise with float atomics (the reference test passes repeated indexes,
 * tests/test_spherical_harmonics.py:27).  d_camera_pos 3 floats.  d_positions / d_camera_pos may
 * be NULL.  If slot_of (n int32: row of Gaussian i in the index list, or -1; from gs_project_fwd)
 * is given, the dense gradient is written in one pass over all n Gaussians (no memset, no atomics) and
 * grad_out may be strided: row i of the upstream gradient is grad_out + i*grad_out_stride
 * (grad_out_stride <= 0 means `channels`).  fwd_out (optional, same striding rule) is the forward's
 * output: when given and neither d_positions nor d_camera_pos is requested, the clamp mask is taken
 * from it (0 < out < 1) and the coefficients are not re-read.
 */
int gs_sh_fwd(int64_t v, const int32_t* v_dev, int32_t channels, int32_t degree, const float* params,
              const float* positions, const int64_t* indexes, const float* camera_pos, float* out,
              int32_t out_stride, void* stream);
/* Sharded frame (no reference counterpart): gs_sh_fwd for the rows whose splat can reach a tile row of
 * `shard` (points2d (v,7) from gs_project_fwd; a superset of what gs_map_prepare lists for that shard); the other rows
 * of `out` receive 0.5 ("not clamped").  shard == NULL evaluates the rows of the whole image's splats. */
/* Sharded frame, the colours of a LIST of rows (the mapper's touched list, gs_map_touched_list): row ids rows[0 ..
 * *rows_count) (both on the device; v = capacity of the list), out row = the listed row, nothing else is written. */
int gs_sh_fwd_rows(int64_t v, const int32_t* rows, const int32_t* rows_count, int32_t channels, int32_t degree,
                   const float* params, const float* positions, const int64_t* indexes, const float* camera_pos,
                   float* out, int32_t out_stride, void* stream);
int gs_sh_fwd_shard(int64_t v, const int32_t* v_dev, int32_t channels, int32_t degree, const float* params,
                    const float* positions, const int64_t* indexes, const float* camera_pos, const float* points2d,
                    int32_t height, const GsRasterConfig* cfg, const GsRowShard* shard, float* out,
                    int32_t out_stride, void* stream);
/* Sharded frame: split gs_raster_bwd's gradient rows (v, gs_grad_row_floats(F)) into the two packed arrays the ranks
 * sum: splat_out (v, 7 + colour_col0) = columns [0, 7 + colour_col0) and colour_out (v, F - colour_col0) = the feature
 * columns from colour_col0 on.  features (optional, (v,F): the forward's SH colours of THIS rank) zeroes the colour
 * gradient of clamped channels before the sum -- required with gs_sh_fwd_shard, whose other rows are 0.5. */
int gs_shard_pack_grads(int64_t v, int32_t num_features, int32_t colour_col0, const float* grad_rows,
                        const float* features, float* colour_out, float* splat_out, void* stream);
/* Sharded frame, sparse exchange: a rank's partial gradients cover the splats that can reach its rows only (7/8 of
 * the rows an 8-rank all-reduce sums are zeros on every rank).  gs_shard_pack_sparse writes one entry of 8 + F words
 * per touched splat: [row id (int32 bits), d splat (7), d features (F)] with the clamp mask of gs_shard_pack_grads
 * applied (features (v,F) optional); `touched` (m int32 rows of the gradient-row buffer) is the mapper's list
 * (gs_map_touched_offset) or any list of distinct rows.  gs_shard_add_sparse adds m entries into the two packed
 * arrays gs_shard_pack_grads would have filled, splat_out (v, 7 + colour_col0) and colour_out (v, F - colour_col0):
 * plain read-modify-write, the rows of ONE call are distinct, so calling it once per source rank in rank order
 * gives every rank the same sums bit for bit. */
int gs_shard_pack_sparse(int64_t m, const int32_t* touched, int32_t num_features, int32_t colour_col0,
                         const float* grad_rows, const float* features, float* entries, void* stream);
int gs_shard_add_sparse(int64_t m, const float* entries, int32_t num_features, int32_t colour_col0, int64_t v,
                        float* colour_out, float* splat_out, void* stream);
/* All `world` lists at once, for lists whose row ids ASCEND (gs_map_touched_list): entries_host / counts_host are HOST
 * arrays of `world` device pointers / entry counts (padding beyond a list's count is not read).  One pass: every row of
 * colour_out / splat_out is WRITTEN (zeros where no list has it -- the buffers need not be cleared), the lists are
 * summed in rank order inside each 256-row tile, so every rank gets the same bits, as with gs_shard_add_sparse list by
 * list.  row_range (optional, device int32[2], from gs_map_touched_list's owned_rows): only the 256-row tiles that
 * meet [first, last) are written (sharded gradients: nothing else is read).  tmp: 4 * world * (ceil(v / 256) + 1) bytes. */
int gs_shard_merge_sparse(int32_t world, const float* const* entries_host, const int64_t* counts_host,
                          int32_t num_features, int32_t colour_col0, int64_t v, float* colour_out, float* splat_out,
                          const int32_t* row_range, void* tmp, int64_t tmp_bytes, void* stream);
int gs_sh_bwd(int64_t n, int64_t v, int32_t channels, int32_t degree, const float* params, const float* positions,
              const int64_t* indexes, int32_t indexes_unique, const int32_t* slot_of, const float* camera_pos,
              const float* grad_out, int32_t grad_out_stride, const float* fwd_out, int32_t fwd_out_stride,
              float* d_params, float* d_positions, float* d_camera_pos, void* stream);
/* Row-compact SH adjoint: gs_sh_bwd's dense single pass for the v visible rows only.  indexes (v) int64, distinct
 * (gs_project_fwd's list); grad_out / fwd_out are read at row i (striding and the clamp-mask shortcut as in gs_sh_bwd);
 * d_params (v,C,D) and the optional d_positions (v,3) receive ROW i = what gs_sh_bwd writes to row indexes[i], bit for
 * bit; nothing is written for the culled Gaussians.  d_camera_pos (3, optional) is zeroed inside, then summed. */
int gs_sh_bwd_rows(int64_t n, int64_t v, int32_t channels, int32_t degree, const float* params, const float* positions,
                   const int64_t* indexes, const float* camera_pos, const float* grad_out, int32_t grad_out_stride,
                   const float* fwd_out, int32_t fwd_out_stride, float* d_params, float* d_positions,
                   float* d_camera_pos, void* stream);

/* --------------------------------------------------------------- tile mapper (a5 - a10) --
 * Fused path (what map_to_tiles runs).  replaces mapper/tile_mapper.py:169-196 as a whole:
 *   gs_map_prepare: OBB tile query per Gaussian (taichi_lib/grid_query.py:10-91) -> per-tile
 *     histogram -> exclusive scan -> tile_ranges (T,2) (empty tiles (0,0), :186) and
 *     counts_out[0] = K, counts_out[1] = largest tile population (device int32[4], see below).
 *   gs_map_finish: re-runs the query, buckets (depth key, index) pairs by tile, then sorts each
 *     tile's bucket on the composite (depth bits, Gaussian index): exactly the order of the
 *     reference's stable 48-bit radix sort of (tile<<32 | depth bits) in generation order
 *     (:34-40, :113-155).  overlap_to_point (K) int32; sorted_keys (K) uint64, optional (NULL),
 *     receives the reference's key layout for verification.
 * image size is the UNPADDED (width,height); padding to a tile multiple is internal (:18-22).
 * depth: (v) f32, non-negative (ndc depth).  use_depth16: key layout of :53-59.
 * scratch: gs_map_scratch_bytes(v, num_tiles), the SAME buffer for both calls (prepare leaves the
 * region ordering in it); pair_scratch: K * 8 bytes.
 * Asynchronous use (no host read-back between the calls): v may be a capacity with the live count in
 * v_dev (device int32); k_capacity > 0 bounds the pair / overlap buffers -- tiles that would run
 * past it are dropped and counts_out[2] is set to 1 so that the caller can retry with more room;
 * counts_out is int32[4] = {K, fullest tile, overflow flag, heavy tiles (see gs_raster_fwd; 0 without tile_order)};
 * max_tile_count <= 0 in
 * gs_map_finish means "not read back": its magnitude is only a hint for sizing the per-tile sort
 * (0 = no hint); fuller tiles are still sorted.  tile_order (optional, T int32) receives the tiles by
 * descending population: a launch order for gs_raster_fwd / gs_raster_bwd (heaviest tiles first).
 * counts_host (optional): device-accessible pinned HOST memory, int32[6]; the scan kernel stores the four
 * counts_out words, then *v_dev (0 without v_dev) and then M, the number of "touched" Gaussians (those whose
 * candidate tile span reaches an owned tile row: the whole list the mapper works on), there as well, so a caller that
 * has to size buffers from K waits for an event recorded behind gs_map_prepare and reads them -- no device-to-host
 * copy launch.  The touched list itself -- M int32 rows of `points`, grouped by screen region -- is left in `scratch` at
 * byte offset gs_map_touched_offset(v, num_tiles): a sharded frame exchanges the gradient rows of exactly these
 * splats (gs_shard_pack_sparse).
 * shard (optional, host pointer, read during the call): only the owned tile rows are mapped; num_tiles in
 * gs_map_scratch_bytes and the T of tile_ranges / tile_order are then the LOCAL tile count, sorted_keys carry local
 * tile ids.  Tile decisions are computed in full-image coordinates: the tiles of a shard get exactly the lists the
 * unsharded call gives them.
 */
int64_t gs_map_scratch_bytes(int64_t v, int64_t num_tiles);
int64_t gs_map_touched_offset(int64_t v, int64_t num_tiles);
/* The touched rows in ASCENDING order (the list at gs_map_touched_offset is grouped by screen region): read from the
 * scratch gs_map_prepare has filled, written to touched_out (room for v int32; M of them are written, M = counts_host[5]).
 * Ascending rows make the gather of gs_shard_pack_sparse and the read-modify-write of gs_shard_add_sparse walk memory
 * forwards.  With owner_counts (world int64, optional): rank r owns the Gaussians [r chunk, (r + 1) chunk), chunk =
 * ceil(n / world), and since rows ascend with the Gaussian index (indexes (v) int64 from gs_project_fwd) the rows of one
 * owner are contiguous in the list -- owner_counts[r] = how many belong to owner r: the send counts of the all-to-all of
 * grad_mode "sharded".  count_out (optional, device int32) receives M.  owned_rows (optional, device int32[2], with
 * owner_counts): the row range [first, last) of the visible list whose Gaussians rank `owner` owns. */
int gs_map_touched_list(int64_t v, const int32_t* v_dev, int64_t num_tiles, const void* scratch, int64_t scratch_bytes,
                        int32_t* touched_out, int32_t* count_out, const int64_t* indexes, int64_t n, int32_t world,
                        int64_t* owner_counts, int32_t owner, int32_t* owned_rows, void* stream);
int gs_map_prepare(int64_t v, const int32_t* v_dev, const float* points, int32_t width, int32_t height,
                   const GsRasterConfig* cfg, int64_t k_capacity, int32_t* tile_ranges, int32_t* counts_out,
                   int32_t* counts_host, int32_t* tile_order, const GsRowShard* shard, void* scratch,
                   int64_t scratch_bytes, void* stream);
int gs_map_finish(int64_t v, const int32_t* v_dev, int64_t k, int32_t max_tile_count, const float* points,
                  const float* depth, int32_t width, int32_t height, const GsRasterConfig* cfg, int32_t use_depth16,
                  const int32_t* tile_ranges, int32_t* overlap_to_point, uint64_t* sorted_keys, void* pair_scratch,
                  const GsRowShard* shard, void* scratch, int64_t scratch_bytes, void* stream);

/* Diagnostic: the device forms of the two functions of include/gs_detmath.h the mapper's integer decisions rest on
 * (correctly rounded sqrt, deterministic ln), element-wise, so that a test can hold them bit for bit against the
 * host forms the CPU oracle is built from.  Either output may be NULL. */
int gs_selftest_detmath(int64_t n, const float* x, float* sqrt_out, float* log_out, void* stream);

/* Reference-shaped primitives (the same pipeline stage by stage, as the reference runs it). */

/* replaces: mapper/tile_mapper.py:74-84 tile_overlaps_kernel.  counts (v) int32. */
int gs_tile_count(int64_t v, const float* points, int32_t width, int32_t height, const GsRasterConfig* cfg,
                  int32_t* counts, void* stream);
/* replaces: cuda_lib.full_cumsum (cuda_lib/__init__.py:16-25, full_cumsum.cu:17-67).
 * out has n+1 entries; out[n] is the total (read it back from there).  scratch: gs_cumsum_scratch_bytes(n). */
int64_t gs_cumsum_scratch_bytes(int64_t n);
int gs_full_cumsum_i32(int64_t n, const int32_t* in, int32_t* out, void* scratch, int64_t scratch_bytes,
                       void* stream);
/* replaces: mapper/tile_mapper.py:113-144 generate_sort_keys_kernel.  keys (K) uint64 (the u32
 * depth16 key is zero-extended), values (K) int32, in generation order. */
int gs_tile_emit_keys(int64_t v, const float* points, const float* depth, const int32_t* offsets, int32_t width,
                      int32_t height, const GsRasterConfig* cfg, int32_t use_depth16, uint64_t* keys,
                      int32_t* values, void* stream);
/* replaces: cuda_lib.radix_sort_pairs (cuda_lib/__init__.py:28-35, radix_sort_pairs.cu:8-70):
 * stable ascending LSD radix sort of (key,value) pairs on key bits [begin_bit,end_bit)
 * (end_bit <= 0 means all bits).  key_bytes 4 or 8.  Outputs in keys_out / values_out; the inputs
 * are preserved.  scratch: gs_sort_scratch_bytes(k, key_bytes). */
int64_t gs_sort_scratch_bytes(int64_t k, int32_t key_bytes);
int gs_radix_sort_pairs(int64_t k, int32_t key_bytes, const void* keys_in, const int32_t* values_in, void* keys_out,
                        int32_t* values_out, int32_t begin_bit, int32_t end_bit, void* scratch,
                        int64_t scratch_bytes, void* stream);
/* replaces: cuda_lib.segmented_sort_pairs (cuda_lib/segmented_sort_pairs.cu:8-78; exported by the reference's
 * native module, not called on the render path): ascending sort of the pairs inside each segment
 * [start_offsets[s], end_offsets[s]) (int64, device); key_bytes 2 or 4 (signed keys), int32 values; stable.
 * Positions outside every segment are not written.  scratch: 8 bytes per item. */
int gs_segmented_sort_pairs(int64_t num_items, int32_t key_bytes, const void* keys, const int32_t* values,
                            void* keys_out, int32_t* values_out, int64_t num_segments, const int64_t* start_offsets,
                            const int64_t* end_offsets, void* scratch, int64_t scratch_bytes, void* stream);
/* replaces: mapper/tile_mapper.py:91-110 find_ranges_kernel (+ zero-init :186). */
int gs_find_ranges(int64_t k, const uint64_t* sorted_keys, int32_t use_depth16, int64_t num_tiles,
                   int32_t* tile_ranges, void* stream);

/* ------------------------------------------------------------- rasterizer (a11 - a13) --
 * replaces: rasterizer/forward.py:25-137 _forward_kernel (allocation contract of
 * rasterizer/function.py:43-76).  points (V,7), features (V,F), tile_ranges (T,2) int32 with
 * T = ceil(W/ts)*ceil(H/ts), overlap_to_point (K) int32.  image (H,W,F), alpha (H,W).
 * visibility (V) must be zero-filled by the caller when cfg->compute_visibility, else may be NULL.
 * tile_order (optional, T int32, a permutation of the tile ids, from gs_map_prepare): launch order;
 * NULL = XCD-contiguous bands.  heavy_tiles (optional, device int32, from gs_map_prepare's counts_out[3]): the
 * first *heavy_tiles tiles of the order are rasterized by four workgroups each (one per 8x8 quadrant; tile_size
 * 16 only, ignored otherwise) so that no single wave walks a very full tile alone.  Results depend on neither.
 * shard (optional, see GsRowShard): tile ids are local, image / alpha hold the owned pixel rows only.
 *
 * Background colour and differentiable weight image (no reference counterpart: the reference composites in torch and
 * marks the weight non-differentiable).  With T = 1 - alpha the transmittance a pixel's walk ended with:
 *   forward:  image_c = sum_i w_i f_ic + T * background[c - background_offset]  for c >= background_offset, composited in
 *             the kernel's epilogue; channels below background_offset (the depth features of a depth render) composite on
 *             0.  background (device, num_features - background_offset floats) may be NULL; alpha is unchanged.
 *   backward: image is the forward's (composited) image; grad_weight (H,W; optional) is dL/d alpha and needs the
 *             forward's alpha image (alpha may be NULL without it).  Both enter through each pixel's initial remaining
 *             colour only, R0 = sum_c image_c g_c - T grad_weight, because dT/d alpha_i = -T / (1 - alpha_i); the
 *             heuristics follow from the corrected dL/d alpha.  dL/d background_c = sum_pixels g_c T is left to the
 *             caller.
 * A background with cfg->use_alpha_blending = 0 returns GS_ERR_UNSUPPORTED, a background_offset outside [0, F) or a
 * grad_weight without alpha GS_ERR_INVALID_ARGUMENT, before any launch.  The _wide and _f64 pairs below take the same
 * arguments with the same meaning.
 */
int gs_raster_fwd(int64_t v, int32_t num_features, const float* points, const float* features,
                  const int32_t* tile_ranges, const int32_t* overlap_to_point, int64_t k, int32_t width,
                  int32_t height, const GsRasterConfig* cfg, const int32_t* tile_order, const int32_t* heavy_tiles,
                  float* image, float* alpha, float* visibility, const GsRowShard* shard, const float* background,
                  int32_t background_offset, void* stream);

/* replaces: rasterizer/backward.py:53-228 _backward_kernel.
 * Per-Gaussian gradients are accumulated with float atomics into ONE row per Gaussian,
 * grad_rows (V, gs_grad_row_floats(F)), 64-byte aligned rows:
 *   [0..7) d(mean.xy, axis.xy, sigma.xy, alpha), [7..7+F) d(features), [7+F, 8+F) point heuristics.
 * (One 64-B segment per (tile, splat) is the shape the memory-side float atomics run fastest at.)
 * The caller zero-fills grad_rows.  gs_raster_bwd_unpack splits rows into the reference's
 * separate tensors (rasterizer/function.py:84-91); any output may be NULL.
 */
int32_t gs_grad_row_floats(int32_t num_features);
int gs_raster_bwd(int64_t v, int32_t num_features, const float* points, const float* features,
                  const int32_t* tile_ranges, const int32_t* overlap_to_point, int64_t k, int32_t width,
                  int32_t height, const GsRasterConfig* cfg, const int32_t* tile_order, const int32_t* heavy_tiles,
                  const float* image, const float* grad_image, const float* alpha, const float* grad_weight,
                  float* grad_rows, const GsRowShard* shard, void* stream);
int gs_raster_bwd_unpack(int64_t v, int32_t num_features, const float* grad_rows, float* grad_points,
                         float* grad_features, float* point_heuristic, void* stream);

/* Wide features: the forward and backward above for 1 <= num_features <= GS_MAX_WIDE_FEATURES (features lifted from
 * 2D models), honouring every GsRasterConfig field gs_raster_fwd / gs_raster_bwd honour.  No tile order, heavy-tile
 * split or row shard.  The forward writes image (H,W,F) and alpha (H,W), and adds into visibility (V) as gs_raster_fwd.
 * The backward adds into the caller's zero-filled grad_points (V,7), grad_features (V,F) and, when
 * cfg->compute_point_heuristic, point_heuristic (V,2); it refuses use_alpha_blending = 0 as gs_raster_bwd does.
 */
int gs_raster_fwd_wide(int64_t v, int32_t num_features, const float* points, const float* features,
                       const int32_t* tile_ranges, const int32_t* overlap_to_point, int64_t k, int32_t width,
                       int32_t height, const GsRasterConfig* cfg, float* image, float* alpha, float* visibility,
                       const float* background, int32_t background_offset, void* stream);
int gs_raster_bwd_wide(int64_t v, int32_t num_features, const float* points, const float* features,
                       const int32_t* tile_ranges, const int32_t* overlap_to_point, int64_t k, int32_t width,
                       int32_t height, const GsRasterConfig* cfg, const float* image, const float* grad_image,
                       const float* alpha, const float* grad_weight, float* grad_points, float* grad_features,
                       float* point_heuristic, void* stream);

/* ------------------------------------------------- plain features (render_gaussians(use_sh=False)) --
 * replaces: `features = gaussians.feature[indexes]` (renderer.py:166) and its index backward, inside the fused frame:
 * gather rows of the (N, C) features into the rasterizer's feature buffer (row stride out_stride, live count
 * optionally in v_dev), and the dense adjoint d_features (N, C): row i = gradient row slot_of[i] (stride
 * grad_out_stride) or zeros for a culled Gaussian.
 */
int gs_feature_gather_fwd(int64_t v, const int32_t* v_dev, int32_t channels, const float* features,
                          const int64_t* indexes, float* out, int32_t out_stride, void* stream);
int gs_feature_gather_bwd(int64_t n, int32_t channels, const int32_t* slot_of, const float* grad_out,
                          int32_t grad_out_stride, float* d_features, void* stream);
/* Row-compact adjoint of the gather: d_features (v, C), row i = the first C columns of gradient row i (stride
 * grad_out_stride, <= 0 means C) -- a strided row copy; the rows belong to the Gaussians of the visible list. */
int gs_feature_gather_bwd_rows(int64_t v, int32_t channels, const float* grad_out, int32_t grad_out_stride,
                               float* d_features, void* stream);

/* ------------------------------------------------------- depth / depth-variance epilogue --
 * replaces: renderer.py:174-180 compute_depth_variance (+ the feature slice at :213-215) for
 * render_depth=True.  image (P, 2+C) rasterized [z, z^2, features], alpha (P): depth = I0/(alpha+eps),
 * depth_var = I1/(alpha+eps) - depth^2, features = I[2:].  Backward assembles grad_image (P, 2+C) from
 * the three upstream gradients (any may be NULL = zero); alpha is non-differentiable.
 */
int gs_depth_split_fwd(int64_t pixels, int32_t channels, const float* image, const float* alpha, float eps,
                       float* features, float* depth, float* depth_var, void* stream);
int gs_depth_split_bwd(int64_t pixels, int32_t channels, const float* depth, const float* alpha, float eps,
                       const float* grad_features, const float* grad_depth, const float* grad_depth_var,
                       float* grad_image, void* stream);

/* --------------------------------------------------- one call per direction --
 * replaces: renderer.py:134-231 render_gaussians as a whole -- project_to_image (:154-157), evaluate_sh_at / the
 * feature gather (:160-166), map_to_tiles + rasterize_with_tiles (render_projected, :183-231), the depth / variance
 * epilogue (:174-180) and the median-depth pass (:203-208) -- and its autograd backward.
 *
 * gs_frame_fwd and gs_frame_bwd enqueue the entry points above, in the order and with the arguments of the
 * stage-by-stage composition (results are bit-identical), from ONE host call each, into ONE caller-provided workspace:
 * gs_frame_layout gives the byte offset of every sub-buffer (-1 = not present for this frame) so that the caller can
 * view them as tensors.  No allocation and no synchronisation inside.
 *   GsFrame (host struct): the frame.  sh_degree -1 = plain (n, channels) features (use_sh=False).  k_capacity (>= 1):
 *     how many (tile, splat) overlaps the workspace holds; the mapper clamps to it and raises the overflow flag
 *     (counts word [6]), in which case the caller runs the frame again with more room.  max_tile_hint: expected
 *     population of the fullest tile (sizes the per-tile sort launches; 0 = none; fuller tiles are still sorted).
 *     prepare_backward: the forward also zero-fills the gradient rows gs_frame_bwd accumulates into (inside the
 *     projection's compaction pass: no fill launch); without it gs_frame_bwd clears its own rows first.
 *   workspace (gs_frame_layout().workspace_bytes): outputs and everything the backward reads.  `counts` is int32[8]:
 *     [0] = V, [4] = K, [5] = fullest tile, [6] = overflow flag, [7] = heavy tiles.  Per-Gaussian buffers are sized
 *     for n rows; V rows are live.  scratch: fwd_scratch_bytes / bwd_scratch_bytes, dead when the call's work has run.
 *   counts_host (optional, pinned host int32[5]) as in gs_map_prepare: {K, fullest tile, overflow, heavy, V}.
 *   counts_event (optional, a hipEvent_t): recorded on `stream` right behind the mapper's scan, i.e. when counts_host is
 *     final -- the caller waits on it for V and K while the sort and the rasterizer are still running.
 *   gs_frame_fwd: background (device, `channels` floats, may be NULL) is composited under the colour channels in the
 *     rasterizer's epilogue (gs_raster_fwd); the depth features of render_depth composite on 0, so depth and depth_var
 *     do not change, and the median-depth pass has no background.
 *   gs_frame_bwd: v, k = the counts read back; grad_image (H, W, C) and, with render_depth, grad_img_depth /
 *     grad_img_var (H, W) -- any may be NULL (zero); grad_weight (local_height x width, may be NULL) is dL/d alpha
 *     (gs_raster_bwd): it reads the workspace's alpha image and needs a grad_image (zeros will do), and the divisor of
 *     depth / depth_var keeps treating alpha as a constant; attached_points (v, 7) / attached_depth (v): gradients the
 *     caller attached to the projected splats / depths themselves (optional).  Outputs: dense parameter gradients
 *     d_position (n,3), d_log_scaling (n,3), d_rotation (n,4), d_alpha_logit (n,1), d_feature (n,C[,D]);
 *     d_T_camera_world (16) / d_projection (4) optional; d_camera_centre (3, optional, ZEROED BY THE CALLER) receives
 *     the SH view direction's gradient with respect to the camera centre.
 *     part (GsFrameBwdPart; NULL = every stage on all rows): run the stages [first_stage, end_stage) of GS_BWD_* only
 *     -- RASTER (clears the gradient rows unless prepare_backward did), COLOURS (SH / feature-gather adjoint from
 *     colour_grads), PROJECT (adds the attached gradients into splat_grads, then the projection adjoint) -- on the
 *     Gaussians [row_begin, row_end), whose gradients fill outputs of row_end - row_begin rows.  A sharded frame
 *     exchanges its partial gradients between RASTER and COLOURS, so no call of it may run both (a NULL part, which
 *     runs every stage, is refused for a sharded frame).
 *   gs_frame_bwd_rows: gs_frame_bwd with ROW-COMPACT parameter gradients (sparse visible-row gradients; no reference
 *     counterpart): d_position (v,3), d_log_scaling (v,3), d_rotation (v,4), d_alpha_logit (v,1), d_feature (v,C[,D]),
 *     row i for Gaussian indexes[i] of the frame's visible list (layout.indexes) -- the adjoints are gs_sh_bwd_rows /
 *     gs_feature_gather_bwd_rows and gs_project_bwd_rows, nothing of size n is written.  Same arguments, so a caller
 *     may run RASTER / COLOURS / PROJECT in separate calls.  Refuses a sharded frame and a row sub-range (row_begin,
 *     row_end other than 0, n) with GS_ERR_UNSUPPORTED.  The camera gradients stay dense.
 */
typedef struct GsFrame {
  int64_t n;
  int32_t channels, sh_degree;
  int32_t width, height;          /* the FULL image, also under a shard */
  double near_plane, far_plane;
  int32_t render_depth, use_depth16, render_median_depth, prepare_backward;
  int64_t k_capacity;
  int32_t max_tile_hint;
  int32_t has_shard;
  GsRowShard shard;
  GsRasterConfig cfg;
  /* render_depth: cfg.forward_cut for the rasterizer call that blends [z, z^2, features] -- the caller divides its
   * forward_cut by far^2 (GsRasterConfig.forward_cut above); the mapper and the median-depth pass use cfg as it is */
  float depth_forward_cut;
  /* Sharded frame with a sparse exchange (has_shard; 0 = none): the number of ranks.  The forward then also leaves the
   * ascending list of the touched rows in the workspace (layout.touched; count in counts[1]; per-owner counts in
   * layout.owner_counts; the row range of the Gaussians rank exchange_rank owns in counts[2..3]) and evaluates SH
   * colours for exactly those rows (gs_sh_fwd_rows; every other colour is 0.5) instead of testing every row against
   * the rank's rows (gs_sh_fwd_shard). */
  int32_t exchange_world, exchange_rank;
} GsFrame;

typedef struct GsFrameLayout {
  int64_t workspace_bytes, fwd_scratch_bytes, bwd_scratch_bytes, stage_bytes;
  /* workspace */
  int64_t counts, camera_pos, points, depth, features, indexes, slot_of, tile_ranges, tile_order, overlap_to_point,
      image, alpha, visibility, out_image, img_depth, img_var, median, grad_rows, touched, owner_counts;
  /* forward scratch */
  int64_t s_ndc_depth, s_pairs, s_median_cover, s_stage;
  /* backward scratch */
  int64_t b_grad_image, b_camera, b_grad_rows;
  int32_t num_features, grad_row_floats, tiles_x, tiles_y, local_height;
} GsFrameLayout;

/* Optional per-stage timing of the frame calls: stage_events is a HOST array of 2 * GS_FWD_STAGES (gs_frame_fwd) or
 * 2 * GS_BWD_STAGES (gs_frame_bwd, gs_frame_bwd_rows) hipEvent_t handles; entry 2 k is recorded in front of stage k and
 * 2 k + 1 behind it, on `stream`; NULL entries (or a NULL array) are skipped.  This is how a caller measures one kernel's launch time with HIP
 * events on the launch stream although the whole direction is one call (bench.py's roofline). */
enum { GS_FWD_PROJECT = 0, GS_FWD_COLOURS, GS_FWD_MAP_PREPARE, GS_FWD_MAP_FINISH, GS_FWD_RASTER, GS_FWD_STAGES };
enum { GS_BWD_RASTER = 0, GS_BWD_COLOURS, GS_BWD_PROJECT, GS_BWD_STAGES };

typedef struct GsFrameBwdPart {
  int32_t first_stage, end_stage;  /* GS_BWD_* */
  const float* colour_grads;       /* NULL: the gradient rows' colour columns (7 + F - channels, row stride RS) */
  float* splat_grads;              /* NULL: the gradient rows (splat columns 0..6, depth features 7..8) */
  int32_t colour_stride, splat_stride;
  int64_t row_begin, row_end;
} GsFrameBwdPart;

int gs_frame_layout(const GsFrame* frame, GsFrameLayout* layout);
int gs_frame_fwd(const GsFrame* frame, const float* position, const float* log_scaling, const float* rotation,
                 const float* alpha_logit, const float* feature, const float* T_camera_world, const float* projection,
                 void* workspace, int64_t workspace_bytes, void* scratch, int64_t scratch_bytes, int32_t* counts_host,
                 void* counts_event, void* const* stage_events, const float* background, void* stream);
int gs_frame_bwd(const GsFrame* frame, const float* position, const float* log_scaling, const float* rotation,
                 const float* alpha_logit, const float* feature, const float* T_camera_world, const float* projection,
                 void* workspace, int64_t workspace_bytes, void* scratch, int64_t scratch_bytes, int64_t v, int64_t k,
                 const float* grad_image, const float* grad_img_depth, const float* grad_img_var,
                 const float* grad_weight, const float* attached_points, const float* attached_depth,
                 float* d_position, float* d_log_scaling, float* d_rotation, float* d_alpha_logit, float* d_feature,
                 float* d_T_camera_world, float* d_projection, float* d_camera_centre, void* const* stage_events,
                 const GsFrameBwdPart* part, void* stream);
int gs_frame_bwd_rows(const GsFrame* frame, const float* position, const float* log_scaling, const float* rotation,
                      const float* alpha_logit, const float* feature, const float* T_camera_world,
                      const float* projection, void* workspace, int64_t workspace_bytes, void* scratch,
                      int64_t scratch_bytes, int64_t v, int64_t k, const float* grad_image, const float* grad_img_depth,
                      const float* grad_img_var, const float* grad_weight, const float* attached_points,
                      const float* attached_depth, float* d_position, float* d_log_scaling, float* d_rotation,
                      float* d_alpha_logit, float* d_feature, float* d_T_camera_world, float* d_projection,
                      float* d_camera_centre, void* const* stage_events, const GsFrameBwdPart* part, void* stream);

/* ------------------------------------------------------------------- Morton ordering --
 * replaces: misc/morton_sort.py:78-88 code_points64_kernel (Grid.morton_code64, :37-66).  points (n,3);
 * lower_host: 3 floats on the HOST (the grid origin, a min-reduction the caller already has);
 * cell = clamp((p - lower)/inc, 0, size-1), size <= 2^21; codes (n) uint64.  Sorting the codes with
 * gs_radix_sort_pairs gives misc/morton_sort.py:121-126 argsort.
 */
int gs_morton_codes64(int64_t n, const float* points, const float* lower_host, float inc, int32_t size,
                      uint64_t* codes, void* stream);

/* ------------------------------------------------ sparse / fractional optimizer step (8f-3) --
 * replaces: optim/fractional_adam.py:7-85 and optim/fractional_laprop.py scalar_kernel / vector_kernel.
 * For each visible row i (idx = indexes[i], int64) with fractional weight weight[i]: update the running
 * moments m, v of row idx in place and write lr_step (rows, dims).  laprop: 0 = Adam, 1 = LaProp;
 * vector_group: 0 = per-element second moment v (N,dims), 1 = one v per row (N) from |g|^2.
 * m (N,dims), total_weight (N), grad (N,dims).
 * Optional fusions (each may be NULL): row_scale (rows) multiplies the gradient of visible row i
 * (optim/visibility_aware.py:100-103); param (N,dims) applies the step in place,
 * param[idx] -= lr_step * (1 - exp(-2 weight)) * mask_lr[j] * point_lr[idx] (optim/fractional.py:31-32, :57-63,
 * :139-146; mask_lr (dims), point_lr (N) optional), in which case lr_step itself may be NULL.
 */
/* replaces: optim/visibility_aware.py:24-31 (update_visibility) + :93-103 of VisibilityOptimizer.step for the visible
 * rows (indexes unique): running_vis[idx] <- (v^4 + (running^4 - v^4) vis_beta)^(1/4); weight[i] = v / max(running, 1e-12);
 * total_weight[idx] += weight[i]; row_scale[i] = grad_scale / (v + vis_smooth)  (the latter two feed gs_optim_step). */
int gs_optim_visibility_weights(int64_t rows, const int64_t* indexes, const float* visibility, float* running_vis,
                                float* total_weight, float vis_beta, float grad_scale, float vis_smooth, float* weight,
                                float* row_scale, void* stream);
int gs_optim_step(int32_t laprop, int32_t vector_group, int64_t rows, int32_t dims, const int64_t* indexes,
                  const float* weight, float* m, float* v, const float* total_weight, const float* grad, float lr,
                  float beta1, float beta2, float eps, int32_t bias_correction, float* lr_step,
                  const float* row_scale, float* param, const float* mask_lr, const float* point_lr, void* stream);
/* The same step from a ROW-COMPACT gradient (the values of a frame's sparse visible-row gradient): grad (grad_count,
 * dims); visible row i reads row grad_rows[i] of it (int32; NULL: row i, then grad_count >= rows; -1: the gradient of
 * that row is zero, which is what a dense gradient holds for it).  Everything else as gs_optim_step, and the same
 * arithmetic: fed the same numbers the two leave the same bits.
 * gs_optim_grad_rows fills such a grad_rows: the position of indexes[i] in grad_indexes (grad_count int64, ASCENDING
 * and distinct -- a frame's points_in_view), or -1; one binary search per row, no host copy, no sort. */
int gs_optim_grad_rows(int64_t rows, const int64_t* indexes, int64_t grad_count, const int64_t* grad_indexes,
                       int32_t* grad_rows, void* stream);
int gs_optim_step_rows(int32_t laprop, int32_t vector_group, int64_t rows, int32_t dims, const int64_t* indexes,
                       const float* weight, float* m, float* v, const float* total_weight, const float* grad,
                       int64_t grad_count, const int32_t* grad_rows, float lr, float beta1, float beta2, float eps,
                       int32_t bias_correction, float* lr_step, const float* row_scale, float* param,
                       const float* mask_lr, const float* point_lr, void* stream);

/* ------------------------------------------------------------------- row lists of several views (rows.hip)
 * A step over a batch of views: each view's backward lists its visible rows ascending and distinct, so the index list
 * of a gradient summed over B backward passes is a concatenation of at most B strictly ascending RUNS.  The three entry
 * points below find the runs, sum the value rows of the runs for the rows of a step, and form the union of the views'
 * row lists, without a sort.  An empty call (count == 0, rows == 0, n == 0) writes nothing and returns 0. */
#define GS_ROWS_MAX_RUNS 16

/* rows (count int64) seen as the concatenation of its maximal STRICTLY ascending runs: a run starts at 0 and at
 * every i with rows[i] <= rows[i-1].  *run_count (device) = the true number of runs, also when it exceeds max_runs;
 * run_starts (device, max_runs + 1) = the starts of the first min(runs, max_runs) runs, ascending, followed by the
 * start of the next run or `count` (and `count` in every entry behind that).  1 <= max_runs <= GS_ROWS_MAX_RUNS. */
int gs_rows_find_runs(int64_t count, const int64_t* rows, int32_t max_runs, int64_t* run_starts,
                      int32_t* run_count, void* stream);

/* out (rows, dims) = for each indexes[i] the sum, IN RUN ORDER, of the value rows that list it (one binary search
 * per run; a strictly ascending run lists a row at most once); zeros where no run lists it.  runs is the host's
 * copy of *run_count, 0 <= runs <= GS_ROWS_MAX_RUNS; run_starts holds runs + 1 entries (entries outside
 * [0, grad_count] are clamped into it); grad_values (grad_count, dims) contiguous.  The result is a deterministic
 * function of the inputs: the same bits on every call. */
int gs_rows_sum_runs(int64_t rows, const int64_t* indexes, int32_t runs, const int64_t* run_starts,
                     int64_t grad_count, const int64_t* grad_indexes, int32_t dims, const float* grad_values,
                     float* out, void* stream);

/* ascending distinct union of rows (count int64, any order, repeats allowed) inside [0, n): a bitmap of n bits in
 * scratch (mark, word-popcount scan, emit).  Entries outside [0, n) are skipped.  union_rows has capacity
 * min(count, n); *union_count on the device.  scratch: 16-byte aligned.  n < 2^31. */
int64_t gs_rows_union_scratch_bytes(int64_t n);
int gs_rows_union(int64_t n, int64_t count, const int64_t* rows, int64_t* union_rows, int32_t* union_count,
                  void* scratch, int64_t scratch_bytes, void* stream);

/* A batch of views taken as a batch (render_views): every view's frame holds slot_of (n int32: the compact row of
 * Gaussian i in that view, negative = not in view; GsFrameLayout.slot_of), which is what the two entry points above
 * search for.  Up to GS_VIEWS_MAX views; an empty call (n == 0, rows == 0, views == 0) writes nothing and returns 0,
 * except gs_views_sum_rows with views == 0 and rows > 0, which writes zeros. */
#define GS_VIEWS_MAX 16

/* ascending distinct union of the views: row r is listed iff slot_of[r] >= 0 in some view.  slot_of_host: a HOST array
 * of `views` device pointers.  One streaming pass over the tables (4 * views * n bytes) builds the bitmap without
 * atomics; scan and emit as gs_rows_union.  union_rows: room for the union (n rows, or the sum of the views' visible
 * counts, always suffice); *union_count on the device.  scratch: 16-byte aligned.  n < 2^31. */
int64_t gs_views_union_scratch_bytes(int64_t n);
int gs_views_union(int64_t n, int32_t views, const int32_t* const* slot_of_host, int64_t* union_rows,
                   int32_t* union_count, void* scratch, int64_t scratch_bytes, void* stream);

/* one view's row-compact values: row slot_of[i] of `values` (count rows, `stride` >= dims floats apart) belongs to
 * Gaussian i */
typedef struct GsViewRows {
  const int32_t* slot_of;
  const float* values;
  int64_t count;
  int32_t stride;
} GsViewRows;

/* out (rows, dims) = for each indexes[i] the sum over the views, IN VIEW ORDER from 0.0f, of
 * values_b[slot_of_b[indexes[i]] * stride_b + 0 .. dims); a view whose slot is < 0 or >= count_b is skipped (nothing
 * is read behind a view's values), a view with count 0 is never read.  The arithmetic of the sequential
 * acc[rows_b] += values_b: the same bits on every call.  view_rows_host: a HOST array of `views` entries, passed to
 * the kernel by value.  indexes[i] must lie inside the tables (negative entries give zeros).  16-byte accesses when
 * dims and every stride are multiples of 4 floats and every values pointer and `out` are 16-byte aligned. */
int gs_views_sum_rows(int64_t rows, const int64_t* indexes, int32_t views, const GsViewRows* view_rows_host,
                      int32_t dims, float* out, void* stream);

/* ---------------------------------------------------------------------- densification --
 * Changing the number of Gaussians (the reference does it in torch, optim/parameter_class.py __getitem__ and
 * append_tensors): a plan says which source row every output row comes from, one launch moves every per-row table by
 * it, a second one places the children of split rows, and a per-row table of statistics collects what the selection
 * thresholds.  Selection itself (top-k, thresholds) is the caller's. */
#define GS_DENSIFY_CHILDREN_MAX 8
#define GS_MOVE_COLUMNS_MAX 32
#define GS_DENSIFY_STATS 6

/* The plan.  prune, split, clone: n bytes each, non-zero = set, NULL = none set.  Per row prune wins over split, split
 * over clone: a pruned row disappears, a split row disappears and yields `children` (1 .. GS_DENSIFY_CHILDREN_MAX) new
 * rows, a cloned row stays and yields one new row, every other row stays.  src_of (capacity int32) = the source row
 * of every output row, in this order, which callers may rely on:
 *   the kept rows ascending (the rows neither pruned nor split: the order of a boolean index),
 *   then the clones, ascending by parent,
 *   then the children, parent-major: the `children` rows of a parent are adjacent, parents ascend.
 * counts (4 int32 on the device) = kept, clones, split parents, rows = kept + clones + children * split parents; they
 * are right also when rows > capacity: entries at or behind `capacity` are not written.  No atomics: the same masks
 * give the same plan.  n * max(2, children) < 2^31.  scratch: gs_densify_plan_scratch_bytes(n), 16-byte aligned.
 * n == 0: nothing is written. */
int64_t gs_densify_plan_scratch_bytes(int64_t n);
int gs_densify_plan(int64_t n, const uint8_t* prune, const uint8_t* split, const uint8_t* clone, int32_t children,
                    int64_t capacity, int32_t* src_of, int32_t* counts, void* scratch, int64_t scratch_bytes,
                    void* stream);

/* one column of a table: rows of row_bytes contiguous bytes (a positive multiple of 4; src and dst 4-byte aligned) */
typedef struct GsMoveColumn {
  const void* src;
  void* dst;        /* `rows` rows; must not overlap src */
  int32_t row_bytes;
  int64_t copy_rows; /* 0 .. rows: dst rows from here on are zero-filled (fresh optimizer state) */
} GsMoveColumn;

/* For every column and every output row j < rows: dst[j] = src[src_of[j]] if j < copy_rows, else zero bytes.  One
 * launch for all columns; columns_host: a HOST array of `columns` (0 .. GS_MOVE_COLUMNS_MAX) entries, passed to the
 * kernel by value.  Rows move as bytes (NaN payloads, -0.0 and denormals survive), with 16-byte accesses in a column
 * whose row_bytes, src and dst are all multiples of 16 and 4-byte accesses otherwise.  src_of[j] must be a row of src
 * (not checked).  rows < 2^31, and a column has fewer than 2^32 - 2^19 access units (rows * row_bytes / 16, or / 4),
 * GS_ERR_UNSUPPORTED otherwise.  rows == 0 or columns == 0: returns 0. */
int gs_table_move_rows(int64_t rows, const int32_t* src_of, int32_t columns, const GsMoveColumn* columns_host,
                       void* stream);

/* The children of split 3D Gaussians.  count = children * split parents rows; parent_of (count int32: the tail of the
 * plan's src_of) indexes the SOURCE tables position (n,3), log_scaling (n,3), rotation (n,4, xyzw).  Child t gets
 *   child_position[t]    = position[p] + R(rotation[p] / |rotation[p]|) (exp(log_scaling[p]) * noise[t])
 *   child_log_scaling[t] = log_scaling[p] - (float)log_shrink          (one float32 subtraction)
 * with p = parent_of[t]; noise (count,3) comes from the caller (the library has no random numbers: the result is a
 * function of the arguments); zero noise leaves the parent's position bits.  child_position / child_log_scaling
 * (count,3): the first child row of the destination tables.  Everything else of a child is its parent's and is already
 * in place after gs_table_move_rows. */
int gs_split3d_children(int64_t count, int32_t children, const int32_t* parent_of, const float* position,
                        const float* log_scaling, const float* rotation, const float* noise, double log_shrink,
                        float* child_position, float* child_log_scaling, void* stream);

/* stats (n, GS_DENSIFY_STATS) float32, updated in place from one view's row-compact results (v rows; row t belongs to
 * Gaussian points_in_view[t]; entries outside [0, n) are skipped):
 *   0  += 1 where visibility[t] > 0 (every listed row when visibility is NULL)
 *   1  += sqrt(gx^2 + gy^2), (gx, gy) = grad2d[t * grad2d_stride + 0 .. 2): the gradient of the projected mean
 *   2  += heuristic[t][0] (prune cost)      3  += heuristic[t][1] (split score)
 *   4  += visibility[t]
 *   5   = max(itself, max(gaussians2d[t][4], gaussians2d[t][5])): the larger sigma of the projected splat (v,7)
 * A NULL input leaves its columns untouched.  The rows of a view are distinct, so the update is a plain
 * read-modify-write without atomics; a list that repeats a row gives undefined sums for that row. */
int gs_densify_accumulate(int64_t n, int64_t v, const int64_t* points_in_view, const float* grad2d,
                          int32_t grad2d_stride, const float* heuristic, const float* visibility,
                          const float* gaussians2d, float* stats, void* stream);

/* ------------------------------------------------------------------- Nearest neighbours --
 * Exact k nearest neighbours of every point of a 3D cloud (the simple-knn step that gives a new Gaussian its first
 * scale; no counterpart in the reference, whose trainers bring their own).  points (n,3) float32; k in 1 .. GS_KNN_MAX.
 *   d2(i, j) = (dx * dx + dy * dy) + dz * dz with d = points[j] - points[i], every operation a single float32 operation
 *   in exactly this order, never contracted: a float32 reimplementation reproduces the result bit for bit.
 * Row i of dist2 / index (n,k) lists the k points j != i with the smallest (d2, j) in lexicographic order, ascending:
 * ties in distance go to the smaller index; the point itself is excluded by index, so a duplicate of it is a neighbour
 * at distance 0.  Entries beyond the n - 1 other points are +inf / -1.  A point with a non-finite coordinate is nobody's
 * neighbour and its own row is all +inf / -1.  index may be NULL.
 * Morton codes of the points in their bounding box, gs_radix_sort_pairs, runs of 256 sorted points with one box each;
 * a wave of 64 queries skips a run whose box is further from the box of its queries than its largest k-th distance
 * (a bound formed by the same float32 operations, so it never exceeds the d2 of a pair it stands for).
 * No allocation, no device-to-host copy, no synchronisation: everything is enqueued on `stream`.  scratch:
 * gs_knn3d_scratch_bytes(n) bytes (0 for n <= 0), 16-byte aligned.  After the call its first ceil(n / 256) int32 hold,
 * per run of queries, how many (wave, run) pairs were scanned rather than skipped, of 4 * (ceil(n / 256) - 1)
 * (a diagnostic for benchmarks).
 * n = 0 returns 0 without touching a pointer.  n < 0, n >= 2^31, k outside 1 .. GS_KNN_MAX, a NULL points / dist2 /
 * scratch or a misaligned scratch: GS_ERR_INVALID_ARGUMENT; a short scratch: GS_ERR_SCRATCH_TOO_SMALL. */
#define GS_KNN_MAX 16
int64_t gs_knn3d_scratch_bytes(int64_t n);
int gs_knn3d(int64_t n, const float* points, int32_t k, float* dist2, int32_t* index, void* scratch,
             int64_t scratch_bytes, void* stream);

/* --------------------------------------------------------------- MCMC densification --
 * The fixed-budget strategy of "3D Gaussian Splatting as Markov Chain Monte Carlo" (no counterpart in the reference):
 * dead rows move onto live rows drawn with probability proportional to opacity, the table grows by the same draw, and
 * every iteration adds opacity-gated noise to the positions.  The library has no random numbers: the 32-bit words of
 * the draws and the noise are arguments, so every result is a function of its arguments.
 *
 * gs_sample_rows: m weighted draws with replacement from n rows, exact and independent of any summation order.
 *   q_i   = (uint32) floor(clamp(weights[i], 0, 1) * 2^24); NaN and negative weights give 0, as does a row whose
 *           exclude byte (n uint8, may be NULL) is non-zero
 *   cum   = the inclusive prefix sum of q in uint64 (total = cum[n - 1] < 2^55)
 *   t_j   = floor(random[j] * total / 2^32), the high 64 bits of (random[j] << 32) * total
 *   out[j] = the first i with cum[i] > t_j: always a row with q_i > 0; random = 2^32 - 1 stays inside the table
 * select (m uint8, may be NULL; needs m == n): draw j happens only where select[j] is non-zero, elsewhere out[j] = j.
 * copies (n int32, may be NULL) is zeroed by the call and then counts, with integer atomics, how often each row was
 * drawn.  total == 0 (no drawable row): every out[j] = j and copies stays 0, so callers see a no-op without a
 * read-back.  No synchronisation.  scratch: gs_sample_rows_scratch_bytes(n) bytes (0 for n <= 0), 16-byte aligned.
 * n = m = 0 returns 0 without touching a pointer.  n or m outside 0 .. 2^31 - 1, select with m != n, draws from an
 * empty table, a NULL weights / scratch (or random / out with m > 0), a misaligned buffer: GS_ERR_INVALID_ARGUMENT; a
 * short scratch: GS_ERR_SCRATCH_TOO_SMALL. */
int64_t gs_sample_rows_scratch_bytes(int64_t n);
int gs_sample_rows(int64_t n, const float* weights, const uint8_t* exclude, int64_t m, const uint32_t* random,
                   const uint8_t* select, int32_t* out, int32_t* copies, void* scratch, int64_t scratch_bytes,
                   void* stream);

/* The correction that keeps the rendered result when a Gaussian of opacity o becomes c + 1 of them (itself and its
 * c = copies[i] copies).  For every row with copies[i] > 0, with n = min(copies[i] + 1, GS_MCMC_N_MAX):
 *   o_new = clamp(1 - (1 - o)^(1 / n), min_opacity, 1 - 2^-23)
 *   denom = sum_{i = 1..n} sum_{k = 0..i-1} C(i - 1, k) (-1)^k o_new^(k + 1) / sqrt(k + 1)
 *   new_alpha_logit[i]   = log(o_new / (1 - o_new))
 *   new_log_scaling[i][] = log_scaling[i][] + (float) log(o / denom)      (one float32 addition per axis)
 * evaluated in float64 from the float32 inputs (min_opacity as the double of the float given) and rounded once; the
 * same sum in float32 is off by 2e-5.  opacity (n), log_scaling (n,3), new_alpha_logit (n), new_log_scaling (n,3).
 * Rows with copies[i] <= 0 are not written.  min_opacity must lie inside (0, 1). */
#define GS_MCMC_N_MAX 51
int gs_mcmc_relocation_values(int64_t n, const float* opacity, const float* log_scaling, const int32_t* copies,
                              float min_opacity, float* new_alpha_logit, float* new_log_scaling, void* stream);

/* Every output row j < rows_out with copies[src_of[j]] > 0 takes the new values of its source src_of[j]: the source
 * itself (src_of[j] = j) and all its copies.  Other rows are not written.  out_alpha_logit (rows_out),
 * out_log_scaling (rows_out,3); src_of[j] must be a row of copies / new_* (not checked). */
int gs_mcmc_apply(int64_t rows_out, const int32_t* src_of, const int32_t* copies, const float* new_alpha_logit,
                  const float* new_log_scaling, float* out_alpha_logit, float* out_log_scaling, void* stream);

/* one table of gs_table_relocate_rows: n rows of row_bytes contiguous bytes (a positive multiple of 4; data 4-byte
 * aligned), changed in place */
#define GS_RELOCATE_COPY 0          /* a selected row j becomes a copy of row src_of[j] */
#define GS_RELOCATE_ZERO 1          /* selected rows that moved (src_of[j] != j) and rows with copies > 0 are zeroed */
#define GS_RELOCATE_ZERO_SOURCES 2  /* only rows with copies > 0 are zero-filled */
typedef struct GsRelocateColumn {
  void* data;
  int32_t row_bytes;
  int32_t mode;
} GsRelocateColumn;

/* The in-place counterpart of gs_table_move_rows for up to GS_MOVE_COLUMNS_MAX tables per launch (columns_host: a HOST
 * array, passed to the kernel by value): select (n uint8), copies (n int32) and src_of (n int32) as gs_sample_rows
 * leaves them.  No row other than those the column's mode names is written; rows move as bytes.  The contract is that
 * a selected row is never a source (copies[j] == 0 and no src_of names it), which gs_sample_rows guarantees with
 * exclude = select: the copy then has no row that is both read and written.  A selected row with
 * src_of[j] == j drew nothing (the table had no drawable row) and is left alone in every mode.  src_of and select may
 * be NULL with ZERO_SOURCES columns only, copies with COPY columns only.  Limits as gs_table_move_rows. */
int gs_table_relocate_rows(int64_t n, const int32_t* src_of, const uint8_t* select, const int32_t* copies,
                           int32_t columns, const GsRelocateColumn* columns_host, void* stream);

/* The per-iteration noise, in place on position (n,3), all float32:
 *   q = rotation / |rotation| (xyzw), R(q) as gs_split3d_children builds it; s = exp(log_scaling)
 *   o = 1 / (1 + exp(-alpha_logit));  g = 1 / (1 + exp(-k ((1 - o) - x0)))
 *   position += R (s^2 * (R^T (noise * (g * scale))))          scale = lr * noise_lr
 * A row whose offset is exactly zero keeps its position bits; that covers zero noise and the gate underflowing to 0
 * (exp overflows: o > 0.89 with k = 100, x0 = 0.995).  Such a row costs its 4 bytes of alpha_logit: nothing else of it
 * is loaded or stored.  rotation must be 16-byte aligned. */
int gs_mcmc_perturb(int64_t n, float* position, const float* log_scaling, const float* rotation,
                    const float* alpha_logit, const float* noise, float scale, float k, float x0, void* stream);

/* --------------------------------------------------- Mip-Splatting: the 3D smoothing filter (mip.hip) --
 * The world-space half of Mip-Splatting (no counterpart in the reference): every Gaussian is low-passed with an
 * isotropic Gaussian sized by the highest rate at which any training camera samples it, and its opacity rescaled so
 * that it keeps its mass.
 *
 * gs_mip_sampling_rate: position (n,3) float32; packed: a device table of `cameras` records of GS_MIP_CAMERA_FLOATS
 * float32 each:
 *   [0..11]  rows 0-2 of T_camera_world, row-major        [12..15] fx, fy, cx, cy
 *   [16..19] lo_x, hi_x, lo_y, hi_y = -m W, (1 + m) W, -m H, (1 + m) H for a margin m, rounded to float32 by the host
 *   [20] near plane   [21] far plane   [22] focal = max(fx, fy)   [23] 0
 * For point p and camera c, every product and sum its own float32 rounding, in this order, never contracted:
 *   xc = ((T00*px + T01*py) + T02*pz) + T03          (yc, zc likewise from rows 1, 2)
 *   u  = fx*xc + cx*zc        v = fy*yc + cy*zc
 *   valid = zc >= near && zc <= far && lo_x*zc <= u && u <= hi_x*zc && lo_y*zc <= v && v <= hi_y*zc
 * A NaN makes a comparison false: a non-finite point is never valid.  rate[i] (n float32) = the maximum over the valid
 * cameras of the correctly rounded focal / zc, 0 when there is none (the largest f / d, the paper's definition; not the
 * smallest depth times one global focal length); seen[i] (n int32) = the number of valid cameras.  A float32
 * restatement reproduces both bit for bit.  One launch, no scratch, no synchronisation.
 * n = 0 returns 0 without touching a pointer.  n < 0, n >= 2^31, cameras outside 0 .. GS_MIP_CAMERAS_MAX, a NULL
 * position / rate / seen (or packed with cameras > 0), a pointer not 4-byte aligned: GS_ERR_INVALID_ARGUMENT. */
#define GS_MIP_CAMERA_FLOATS 24
#define GS_MIP_CAMERAS_MAX 65536
int gs_mip_sampling_rate(int64_t n, const float* position, int32_t cameras, const float* packed, float* rate,
                         int32_t* seen, void* stream);

/* gs_smooth3d_*: per row l = log_scaling (n,3), a = alpha_logit (n), f = filter3d (n) >= 0, a constant:
 *   x_k = f^2 e^{-2 l_k}     l'_k = log(e^{2 l_k} + f^2) / 2     log c = -sum_k log1p(x_k) / 2     a' = logit(sigmoid(a) c)
 *   dL/dl_k = g_l'_k / (1 + x_k) + g_a' x_k / (1 + x_k) / (1 - sigmoid(a) c)        dL/da = g_a' / (1 + e^a (1 - c))
 * i.e. scale' = sqrt(scale^2 + f^2) and opacity' = opacity sqrt(det S / det S').  Evaluated in forms that hold for
 * |l|, |a| <= 40 and f in 0 .. 1e6 (head of mip.hip): every output is finite there.  A row with f == 0 returns l, a and
 * both incoming gradients bit for bit.  The forward saves nothing; the backward recomputes from (l, a, f).
 * Dense backward: grad_log_scaling (n,3), grad_alpha_logit (n), either may be NULL (zero); d_log_scaling (n,3) and
 * d_alpha_logit (n) are written.  Row-compact backward: rows (v int64, rows of the n as a frame's sparse gradient lists
 * them), gradients and outputs (v,3), (v); nothing of size n is written or allocated, a row index outside [0, n) gives
 * a zero row.  The two forms run the same device function and agree bit for bit.  The _f64 forms are the same templated
 * source in double (for gradcheck).  Outputs must not alias inputs.
 * n = 0 (v = 0) returns 0 without touching a pointer.  n or v outside 0 .. 2^31 - 1, v > 0 with n = 0, a NULL buffer
 * other than an incoming gradient, a pointer not aligned to its element: GS_ERR_INVALID_ARGUMENT. */
int gs_smooth3d_fwd(int64_t n, const float* log_scaling, const float* alpha_logit, const float* filter3d,
                    float* out_log_scaling, float* out_alpha_logit, void* stream);
int gs_smooth3d_bwd(int64_t n, const float* log_scaling, const float* alpha_logit, const float* filter3d,
                    const float* grad_log_scaling, const float* grad_alpha_logit, float* d_log_scaling,
                    float* d_alpha_logit, void* stream);
int gs_smooth3d_bwd_rows(int64_t n, int64_t v, const int64_t* rows, const float* log_scaling,
                         const float* alpha_logit, const float* filter3d, const float* grad_log_scaling,
                         const float* grad_alpha_logit, float* d_log_scaling, float* d_alpha_logit, void* stream);
int gs_smooth3d_fwd_f64(int64_t n, const double* log_scaling, const double* alpha_logit, const double* filter3d,
                        double* out_log_scaling, double* out_alpha_logit, void* stream);
int gs_smooth3d_bwd_f64(int64_t n, const double* log_scaling, const double* alpha_logit, const double* filter3d,
                        const double* grad_log_scaling, const double* grad_alpha_logit, double* d_log_scaling,
                        double* d_alpha_logit, void* stream);

/* ------------------------------------------------------------------- float64 operators --
 * The projection, SH and rasterizer in float64, for gradcheck (the reference builds these stages for f64 too,
 * rasterizer/function.py:122, perspective/projection.py:27, spherical_harmonics.py:24-27).  Projection and SH are
 * the f32 kernels' arithmetic instantiated with double and IEEE sqrt / exp / log; the rasterizer states the reference
 * formulas literally, with none of the f32 kernels' reformulations.  Every result is
 * bit-reproducible: no float atomic feeds an output (per-entry records summed in a fixed order).  Scope: no tile
 * order, heavy-tile split, row shard or stride options; features up to GS_MAX_FEATURES; forward_cut does not exist
 * here (the forward blends a tile's whole list, as the reference does). */
typedef struct GsRasterConfigF64 {
  int32_t tile_size;  /* 8, 16 or 32 */
  int32_t antialias;
  int32_t use_alpha_blending;
  int32_t compute_point_heuristic;
  int32_t compute_visibility;
  double clamp_margin;
  double blur_cov;
  double clamp_max_alpha;
  double alpha_threshold;
  double saturate_threshold;
} GsRasterConfigF64;

/* gs_project_fwd / gs_project_bwd in f64 (same tensors, same compaction: points (V,7), depth (V,1), ndc_depth (V,1),
 * indexes (V) int64 ascending, slot_of (n), *num_visible).  Camera gradients (d_T_camera_world 4x4, d_projection 4;
 * either may be NULL) are per-workgroup partials reduced in a fixed order.  grad_points / grad_depth may be NULL. */
int64_t gs_project_f64_scratch_bytes(int64_t n);
int gs_project_fwd_f64(int64_t n, const double* position, const double* log_scaling, const double* rotation,
                       const double* alpha_logit, const double* T_camera_world, const double* projection,
                       int32_t width, int32_t height, double near_plane, double far_plane,
                       const GsRasterConfigF64* cfg, double* points, double* depth, double* ndc_depth,
                       int64_t* indexes, int32_t* slot_of, int32_t* num_visible, void* scratch,
                       int64_t scratch_bytes, void* stream);
int64_t gs_project_bwd_f64_scratch_bytes(int64_t n);
int gs_project_bwd_f64(int64_t n, const double* position, const double* log_scaling, const double* rotation,
                       const double* alpha_logit, const double* T_camera_world, const double* projection,
                       int32_t width, int32_t height, const GsRasterConfigF64* cfg, const int32_t* slot_of,
                       const double* grad_points, const double* grad_depth, double* d_position,
                       double* d_log_scaling, double* d_rotation, double* d_alpha_logit, double* d_T_camera_world,
                       double* d_projection, void* scratch, int64_t scratch_bytes, void* stream);

/* gs_sh_fwd / gs_sh_bwd in f64: params (n,C,D), positions (n,3), indexes (v) int64 in [0, n), repeats allowed,
 * camera_pos 3 doubles; out (v,C).  The backward writes the dense d_params (n,C,D), d_positions (n,3) (may be NULL)
 * and d_camera_pos (3, may be NULL); a Gaussian listed several times sums its entries in ascending list order. */
int gs_sh_fwd_f64(int64_t v, int32_t channels, int32_t degree, const double* params, const double* positions,
                  const int64_t* indexes, const double* camera_pos, double* out, void* stream);
int64_t gs_sh_bwd_f64_scratch_bytes(int64_t n, int64_t v);
int gs_sh_bwd_f64(int64_t n, int64_t v, int32_t channels, int32_t degree, const double* params,
                  const double* positions, const int64_t* indexes, const double* camera_pos, const double* grad_out,
                  double* d_params, double* d_positions, double* d_camera_pos, void* scratch, int64_t scratch_bytes,
                  void* stream);

/* gs_raster_fwd / gs_raster_bwd in f64 for 1 <= num_features <= GS_MAX_FEATURES.  The tile ranges must be disjoint (as
 * the mapper makes them).  Forward: image (H,W,F), alpha (H,W), visibility (V, may be NULL unless
 * cfg->compute_visibility; written, not added to).  Backward: grad_points (V,7), grad_features (V,F) and, when
 * cfg->compute_point_heuristic, point_heuristic (V,2) are written (zero for splats in no list); use_alpha_blending = 0
 * is refused as in gs_raster_bwd.  scratch: gs_raster_f64_scratch_bytes(v, k, num_features), for either call. */
int64_t gs_raster_f64_scratch_bytes(int64_t v, int64_t k, int32_t num_features);
int gs_raster_fwd_f64(int64_t v, int32_t num_features, const double* points, const double* features,
                      const int32_t* tile_ranges, const int32_t* overlap_to_point, int64_t k, int32_t width,
                      int32_t height, const GsRasterConfigF64* cfg, double* image, double* alpha,
                      double* visibility, const double* background, int32_t background_offset, void* scratch,
                      int64_t scratch_bytes, void* stream);
int gs_raster_bwd_f64(int64_t v, int32_t num_features, const double* points, const double* features,
                      const int32_t* tile_ranges, const int32_t* overlap_to_point, int64_t k, int32_t width,
                      int32_t height, const GsRasterConfigF64* cfg, const double* image, const double* grad_image,
                      const double* alpha, const double* grad_weight, double* grad_points, double* grad_features,
                      double* point_heuristic, void* scratch, int64_t scratch_bytes, void* stream);

/* -------------------------------------------------------------------- photometric loss --
 * (1 - ssim_weight) * mean|x - y| + ssim_weight * (1 - SSIM(x, y)) on channel-last images, x = image (the render),
 * y = target; both (batch, height, width, channels), read through a batch, a row and a pixel stride in ELEMENTS with
 * the channels contiguous (pixel stride >= channels, row stride >= width * pixel stride), so a channel slice or a row
 * view of a larger buffer goes in without a copy.  SSIM: 1-D Gaussian window of odd size 3 .. 15,
 * g[i] = exp(-(i - (ws - 1) / 2)^2 / (2 sigma^2)) normalised to sum 1 in double and rounded to the compute type, applied
 * as g (x) g per channel with zero padding; C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2;
 *   ssim_map = (2 mu_x mu_y + C1)(2 cov + C2) / ((mu_x^2 + mu_y^2 + C1)(var_x + var_y + C2)).
 * The kernels form the second moments on x - c, y - c' with per-tile pivots (csrc/loss.hip), which keeps float32
 * accurate on smooth, flat and nearly equal images.  `valid` != 0: only pixels whose window lies inside the image enter
 * the SSIM mean (needs height, width >= window_size); the map itself does not change.
 *
 * gs_ssim_window: host only; the float32 weights the kernels use.
 * Forward: results (3, device) = [loss, mean|x - y|, mean ssim]; ssim_map (B,H,W,C) and saved_maps (3,B,H,W,C: what the
 * backward needs) are optional (NULL).  With ssim_weight == 0 and neither map the SSIM work is skipped and results[2]
 * is NaN.  scratch: gs_photo_loss_scratch_bytes, 8-byte aligned; the per-workgroup partial sums are added in a fixed order by a second
 * launch, in double: the results repeat bit for bit.
 * Backward: d_image (B,H,W,C, contiguous; written, not accumulated) =
 *   g * (l1_coeff * d mean|x - y| / dx + ssim_coeff * d mean_ssim / dx) + sum_q upstream_map(q) * d ssim_map(q) / dx,
 * g = *grad_loss (device scalar; NULL = 1), upstream_map (B,H,W,C) optional.  The photometric loss is
 * l1_coeff = 1 - ssim_weight, ssim_coeff = -ssim_weight.  sign(0) = 0 in the L1 term.  saved_maps may be NULL when
 * ssim_coeff == 0 and upstream_map == NULL.  Zero pixels: both calls are no-ops returning 0. */
int gs_ssim_window(int32_t window_size, double sigma, float* host_out);
int64_t gs_photo_loss_scratch_bytes(int64_t batch, int64_t height, int64_t width, int64_t channels);
int gs_photo_loss_fwd(int64_t batch, int64_t height, int64_t width, int64_t channels, const float* image,
                      int64_t image_batch_stride, int64_t image_row_stride, int64_t image_pixel_stride,
                      const float* target, int64_t target_batch_stride, int64_t target_row_stride,
                      int64_t target_pixel_stride, int32_t window_size, double sigma, double data_range,
                      double ssim_weight, int32_t valid, float* ssim_map, float* saved_maps, void* scratch,
                      int64_t scratch_bytes, float* results, void* stream);
int gs_photo_loss_bwd(int64_t batch, int64_t height, int64_t width, int64_t channels, const float* image,
                      int64_t image_batch_stride, int64_t image_row_stride, int64_t image_pixel_stride,
                      const float* target, int64_t target_batch_stride, int64_t target_row_stride,
                      int64_t target_pixel_stride, int32_t window_size, double sigma, int32_t valid,
                      const float* saved_maps, const float* upstream_map, const float* grad_loss, double l1_coeff,
                      double ssim_coeff, float* d_image, void* stream);
int gs_photo_loss_fwd_f64(int64_t batch, int64_t height, int64_t width, int64_t channels, const double* image,
                          int64_t image_batch_stride, int64_t image_row_stride, int64_t image_pixel_stride,
                          const double* target, int64_t target_batch_stride, int64_t target_row_stride,
                          int64_t target_pixel_stride, int32_t window_size, double sigma, double data_range,
                          double ssim_weight, int32_t valid, double* ssim_map, double* saved_maps, void* scratch,
                          int64_t scratch_bytes, double* results, void* stream);
int gs_photo_loss_bwd_f64(int64_t batch, int64_t height, int64_t width, int64_t channels, const double* image,
                          int64_t image_batch_stride, int64_t image_row_stride, int64_t image_pixel_stride,
                          const double* target, int64_t target_batch_stride, int64_t target_row_stride,
                          int64_t target_pixel_stride, int32_t window_size, double sigma, int32_t valid,
                          const double* saved_maps, const double* upstream_map, const double* grad_loss,
                          double l1_coeff, double ssim_coeff, double* d_image, void* stream);

/* ------------------------------------------------------- photometric loss, per-pixel weights --
 * The same loss with a weight w >= 0 per pixel (an object, sky or distractor mask, or a confidence), shared by the
 * channels: weight (batch, height, width), read through a batch, a row and a pixel stride in ELEMENTS (pixel stride
 * >= 1, row stride >= width * pixel stride, batch stride >= height * row stride, or 0 = the same weights for every
 * batch entry), so a column or row view of a larger buffer goes in without a copy.  With S the sum of w over every
 * pixel and batch entry and S_v the sum over the pixels that enter the SSIM mean (all of them, or with `valid` those
 * whose window lies inside the image):
 *   L = sum w |x - y| / (channels * S),  M = sum w ssim_map / (channels * S_v),
 *   loss = (1 - ssim_weight) * L + ssim_weight * (1 - M).
 * The map is not changed by the weights: the windows see every pixel of both images.  A term whose weight sum is zero
 * adds nothing to the loss and exactly zero to the gradient, and its part is NaN.  The weights are expected to be
 * finite and non-negative; that is not checked.  weight == NULL runs the unweighted loss (S = batch * height * width).
 *
 * The argument lists are those of the unweighted calls with the weight and its strides after the target's.
 * Forward: results (5, device) = [loss, L, M, S, S_v]; scratch: gs_photo_loss_weighted_scratch_bytes.  The weight sums
 * are added like the other partial sums, in a fixed order and in double: the results repeat bit for bit, all-ones
 * weights give the bits of the unweighted call, and scaling the weights by a power of two changes nothing.
 * Backward: normalisers (2, device) = [S, S_v] as the forward wrote them (results + 3): no value comes back to the
 * host between the two calls.  d_image =
 *   g * (l1_coeff * dL / dx + ssim_coeff * dM / dx) + sum_q upstream_map(q) * d ssim_map(q) / dx;
 * upstream_map is not weighted.  No gradient for the weights.  Zero pixels: both calls are no-ops returning 0. */
int64_t gs_photo_loss_weighted_scratch_bytes(int64_t batch, int64_t height, int64_t width, int64_t channels);
int gs_photo_loss_weighted_fwd(int64_t batch, int64_t height, int64_t width, int64_t channels, const float* image,
                               int64_t image_batch_stride, int64_t image_row_stride, int64_t image_pixel_stride,
                               const float* target, int64_t target_batch_stride, int64_t target_row_stride,
                               int64_t target_pixel_stride, const float* weight, int64_t weight_batch_stride,
                               int64_t weight_row_stride, int64_t weight_pixel_stride, int32_t window_size,
                               double sigma, double data_range, double ssim_weight, int32_t valid, float* ssim_map,
                               float* saved_maps, void* scratch, int64_t scratch_bytes, float* results, void* stream);
int gs_photo_loss_weighted_bwd(int64_t batch, int64_t height, int64_t width, int64_t channels, const float* image,
                               int64_t image_batch_stride, int64_t image_row_stride, int64_t image_pixel_stride,
                               const float* target, int64_t target_batch_stride, int64_t target_row_stride,
                               int64_t target_pixel_stride, const float* weight, int64_t weight_batch_stride,
                               int64_t weight_row_stride, int64_t weight_pixel_stride, const float* normalisers,
                               int32_t window_size, double sigma, int32_t valid, const float* saved_maps,
                               const float* upstream_map, const float* grad_loss, double l1_coeff, double ssim_coeff,
                               float* d_image, void* stream);
int gs_photo_loss_weighted_fwd_f64(int64_t batch, int64_t height, int64_t width, int64_t channels,
                                   const double* image, int64_t image_batch_stride, int64_t image_row_stride,
                                   int64_t image_pixel_stride, const double* target, int64_t target_batch_stride,
                                   int64_t target_row_stride, int64_t target_pixel_stride, const double* weight,
                                   int64_t weight_batch_stride, int64_t weight_row_stride, int64_t weight_pixel_stride,
                                   int32_t window_size, double sigma, double data_range, double ssim_weight,
                                   int32_t valid, double* ssim_map, double* saved_maps, void* scratch,
                                   int64_t scratch_bytes, double* results, void* stream);
int gs_photo_loss_weighted_bwd_f64(int64_t batch, int64_t height, int64_t width, int64_t channels,
                                   const double* image, int64_t image_batch_stride, int64_t image_row_stride,
                                   int64_t image_pixel_stride, const double* target, int64_t target_batch_stride,
                                   int64_t target_row_stride, int64_t target_pixel_stride, const double* weight,
                                   int64_t weight_batch_stride, int64_t weight_row_stride, int64_t weight_pixel_stride,
                                   const double* normalisers, int32_t window_size, double sigma, int32_t valid,
                                   const double* saved_maps, const double* upstream_map, const double* grad_loss,
                                   double l1_coeff, double ssim_coeff, double* d_image, void* stream);

/* ------------------------------------------------ appearance: slicing a bilateral grid (bilagrid.hip) --
 * Per-image colour correction: a grid (batch, 12, grid_l, grid_h, grid_w) of 3x4 affine colour transforms, channel
 * 4 r + c = element (r, c), each batch entry contiguous and `grid_batch_stride` ELEMENTS from the one before (the
 * layout torch's grid_sample takes), sliced at every pixel of a channel-last image (batch, height, width, 3).  For the
 * pixel at column x, row y with colour rgb:
 *   guide = 0.299 r + 0.587 g + 0.114 b, or guide[y, x] when `guide` (batch, height, width) is not NULL
 *   gx = (x + 0.5) / width * (grid_w - 1),  gy = (y + 0.5) / height * (grid_h - 1),  gz = clamp(guide, 0, 1) * (grid_l - 1)
 *   A = trilinear interpolation of the 12 channels at (gz, gy, gx), cell = min(floor(coord), size - 2), 0 for size 1
 *   out = A[:, :3] rgb + A[:, 3]
 * which is grid_sample(mode = bilinear, padding_mode = border, align_corners = True) followed by the affine.  The
 * interpolation is a + (b - a) f along each axis, so an identity grid returns the image bit for bit.  A 1 x 1 x 1
 * grid is one affine colour matrix per image.
 * image and guide are read through a batch, a row and a pixel stride in ELEMENTS (channels contiguous; pixel stride >=
 * 3 for the image, >= 1 for the guide; row stride >= width * pixel stride; batch stride >= height * row stride).
 * Forward: out (batch, height, width, 3), contiguous.
 * Backward: grad_out as out; d_image (as out), d_guide (batch, height, width; only with a guide) and d_grid (as the
 * grid, contiguous) are written, not accumulated; each may be NULL, not all.  d_image holds the gradient through the
 * affine and, without a guide, through the luma; the gradient through gz is zero where the guide is not inside (0, 1).
 * d_grid needs scratch (gs_bilagrid_scratch_bytes, 8-byte aligned; f64 != 0 for the _f64 call): every pixel tile's
 * sums, which a second launch adds in tile order.  Every output of both directions repeats bit for bit.
 * Sizes must be positive (-1).  Any shape with grid_l <= 16 is accepted; the call returns -2 when the 2 x 2 x grid_l
 * nodes around one pixel do not fit in LDS twice (grid_l above 85 in float64), and above 2^22 pixels a side, 2^31 grid
 * elements or 2^31 pixel tiles.  gs_bilagrid_scratch_bytes returns the same negative codes. */
int64_t gs_bilagrid_scratch_bytes(int64_t batch, int64_t height, int64_t width, int64_t grid_l, int64_t grid_h,
                                  int64_t grid_w, int32_t f64);
int gs_bilagrid_slice_fwd(int64_t batch, int64_t height, int64_t width, const float* image,
                          int64_t image_batch_stride, int64_t image_row_stride, int64_t image_pixel_stride,
                          const float* guide, int64_t guide_batch_stride, int64_t guide_row_stride,
                          int64_t guide_pixel_stride, const float* grid, int64_t grid_l, int64_t grid_h,
                          int64_t grid_w, int64_t grid_batch_stride, float* out, void* stream);
int gs_bilagrid_slice_bwd(int64_t batch, int64_t height, int64_t width, const float* image,
                          int64_t image_batch_stride, int64_t image_row_stride, int64_t image_pixel_stride,
                          const float* guide, int64_t guide_batch_stride, int64_t guide_row_stride,
                          int64_t guide_pixel_stride, const float* grid, int64_t grid_l, int64_t grid_h,
                          int64_t grid_w, int64_t grid_batch_stride, const float* grad_out, float* d_image,
                          float* d_guide, float* d_grid, void* scratch, int64_t scratch_bytes, void* stream);
int gs_bilagrid_slice_fwd_f64(int64_t batch, int64_t height, int64_t width, const double* image,
                              int64_t image_batch_stride, int64_t image_row_stride, int64_t image_pixel_stride,
                              const double* guide, int64_t guide_batch_stride, int64_t guide_row_stride,
                              int64_t guide_pixel_stride, const double* grid, int64_t grid_l, int64_t grid_h,
                              int64_t grid_w, int64_t grid_batch_stride, double* out, void* stream);
int gs_bilagrid_slice_bwd_f64(int64_t batch, int64_t height, int64_t width, const double* image,
                              int64_t image_batch_stride, int64_t image_row_stride, int64_t image_pixel_stride,
                              const double* guide, int64_t guide_batch_stride, int64_t guide_row_stride,
                              int64_t guide_pixel_stride, const double* grid, int64_t grid_l, int64_t grid_h,
                              int64_t grid_w, int64_t grid_batch_stride, const double* grad_out, double* d_image,
                              double* d_guide, double* d_grid, void* scratch, int64_t scratch_bytes, void* stream);

/* -------------------------------------------- environment: a cubemap sky behind the render (envmap.hip) --
 * A learnable environment map env (6, map_edge, map_edge, channels), channel-last and contiguous, channels in 1 .. 4,
 * looked up by the view direction of every pixel of a pinhole camera and composited behind a render.  The camera is
 * read on the device: projection = (fx, fy, cx, cy) and T_camera_world = the 4x4 world -> camera matrix, row-major;
 * nothing is read back.  For the pixel at column x, row y (R = map_edge):
 *   d_cam = ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1),  d = Rcw^T d_cam,  Rcw = T_camera_world[:3, :3], taken as a
 *           rotation: the map is at infinity and the translation is not read
 *   a = the axis of the largest |d_i|, ties to the lower index;  face = 2 a + (d_a < 0)
 *   (p, q) = the two other components in ascending axis order, divided by |d_a|   (a = 0: y, z; a = 1: x, z; a = 2: x, y)
 *   u = clamp((p + 1) / 2 * R - 0.5, 0, R - 1) (column),  v = clamp((q + 1) / 2 * R - 0.5, 0, R - 1) (row)
 *   sky = bilinear interpolation of env[face] at (v, u), taps clamped inside the face
 *   out = image + (1 - weight) * sky
 * which is grid_sample(bilinear, border, align_corners = False) on the chosen face.  No sign flips between faces and
 * no filtering across face seams.  A constant map returns the constant bit for bit, weight == 1 the image bit for bit.
 * image (height, width, channels) and weight (height, width) are read through a row and a pixel stride in ELEMENTS
 * (channels contiguous; pixel stride >= channels for the image, >= 1 for the weight; row stride >= width * pixel
 * stride).  They are NULL together: the sky alone.  Forward: out (height, width, channels), contiguous.
 * Backward: grad_out as out.  d_image is grad_out itself and has no kernel.  d_weight (height, width) = -sum_c
 * grad_out_c sky_c, needs weight and env.  d_env (as env, contiguous) is written, not accumulated, exactly zero where
 * no pixel looks: a gather with one sum per texel in an order the shapes fix, no atomics -- every output repeats bit
 * for bit.  d_weight and d_env may each be NULL, not both.  The view direction is not differentiated: no gradient for
 * projection or T_camera_world.  d_env may need scratch (gs_envmap_scratch_bytes, 8-byte aligned; f64 != 0 for the
 * _f64 calls; 0 bytes for most shapes).
 * Sizes below 1 or a NULL buffer where none is allowed: -1; channels outside 1 .. 4, map_edge above 16384 or an image
 * of 2^31 pixels or more: -2; a short scratch: -4; all before any launch.  gs_envmap_scratch_bytes returns the same
 * negative codes. */
int64_t gs_envmap_scratch_bytes(int64_t height, int64_t width, int64_t channels, int64_t map_edge, int32_t f64);
int gs_envmap_fwd(int64_t height, int64_t width, int64_t channels, const float* env, int64_t map_edge,
                  const float* image, int64_t image_row_stride, int64_t image_pixel_stride, const float* weight,
                  int64_t weight_row_stride, int64_t weight_pixel_stride, const float* projection,
                  const float* T_camera_world, float* out, void* stream);
int gs_envmap_bwd(int64_t height, int64_t width, int64_t channels, const float* env, int64_t map_edge,
                  const float* weight, int64_t weight_row_stride, int64_t weight_pixel_stride, const float* projection,
                  const float* T_camera_world, const float* grad_out, float* d_weight, float* d_env, void* scratch,
                  int64_t scratch_bytes, void* stream);
int gs_envmap_fwd_f64(int64_t height, int64_t width, int64_t channels, const double* env, int64_t map_edge,
                      const double* image, int64_t image_row_stride, int64_t image_pixel_stride, const double* weight,
                      int64_t weight_row_stride, int64_t weight_pixel_stride, const double* projection,
                      const double* T_camera_world, double* out, void* stream);
int gs_envmap_bwd_f64(int64_t height, int64_t width, int64_t channels, const double* env, int64_t map_edge,
                      const double* weight, int64_t weight_row_stride, int64_t weight_pixel_stride,
                      const double* projection, const double* T_camera_world, const double* grad_out, double* d_weight,
                      double* d_env, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------- depth: losses against a depth prior with a per-image fit (depth_loss.hip) --
 * depth and prior (batch, height, width), weight the same or NULL (every weight 1), each read through a batch, a row and
 * a pixel stride in ELEMENTS (pixel stride >= 1, row stride >= width * pixel stride, batch stride >= height * row
 * stride; the weight's batch stride may be 0: one weight for every image).  Per image b, with x = depth, or 1 / depth
 * when inverse = 1, p = prior, over the pixels that are not SELECTED OUT -- a pixel is selected out, adds nothing to
 * any sum whatever it holds and gets a gradient of exactly 0, when its weight is not > 0, its depth or prior is not
 * finite, or inverse = 1 and its depth is <= 0:
 *   W = sum w, pm = sum w p / W, xm = sum w x / W, var_p = sum w (p - pm)^2, cov = sum w (p - pm)(x - xm), var_x likewise
 *   kind 0 (L1)       r = x - s p - t,  L_b = sum w |r| / W,  loss = mean over b of L_b, with
 *     align 0 (affine)  s = cov / var_p, t = xm - s pm;  var_p <= 1e-12 sum w p^2:  s = 0, t = xm
 *     align 1 (scale)   s = sum w p x / sum w p^2, t = 0;  sum w p^2 = 0:  s = 0
 *     align 2 (none)    s = 1, t = 0
 *   kind 1 (Pearson)  rho_b = cov / sqrt(var_p var_x), loss = mean over b of 1 - rho_b;  rho_b = 0 with zero gradient
 *                     when W = 0, var_p <= 1e-12 sum w p^2 or var_x <= 1e-12 sum w x^2
 *   kind 2 (fit)      s and t of the align alone; forward only
 * results holds 1 + 3 batch values: the loss (0 for kind 2), then per image L_b, s_b, t_b (kind 1: 1 - rho_b, rho_b,
 * 0); an image with W = 0 adds 0 to an L1 loss and has NaN for its three values.  stats (batch, 18) doubles carries the
 * per-image scalars from the forward to the backward on the device.  Backward: d_depth (batch, height, width),
 * contiguous, = *g_loss (one value on the device) times the exact gradient of the loss, the fit differentiated through:
 *   affine  dL_b / dx_k = w_k / W (sgn r_k - B / W - (A - B pm)(p_k - pm) / var_p),  A = sum w sgn(r) p, B = sum w sgn(r)
 *   scale   dL_b / dx_k = w_k / W (sgn r_k - A p_k / sum w p^2),   none  w_k / W sgn r_k,   sgn 0 = 0
 *   Pearson drho / dx_k = w_k ((p_k - pm) / sqrt(var_p var_x) - rho (x_k - xm) / var_x);   inverse: times -1 / depth_k^2
 * (a degenerate fit drops the term that divides by the vanishing sum).  The float entry points read floats and compute
 * in double up to the one rounding of each output; the _f64 ones are the same templates on double.  Every sum has one
 * order given the shapes, no atomics: outputs repeat bit for bit.  scratch: gs_depth_loss_scratch_bytes, 8-byte aligned.
 * Sizes below 1, a NULL depth / prior / output / stats, overlapping strides: -1; batch * height * width >= 2^31, a batch
 * above 65535 or an unknown kind / align / inverse: -2; a NULL or misaligned scratch: -1, a short one: -4; all before
 * any launch.  gs_depth_loss_scratch_bytes returns the same negative codes. */
int64_t gs_depth_loss_scratch_bytes(int64_t batch, int64_t height, int64_t width);
int gs_depth_loss_fwd(int64_t batch, int64_t height, int64_t width, const float* depth, int64_t depth_batch_stride,
                      int64_t depth_row_stride, int64_t depth_pixel_stride, const float* prior,
                      int64_t prior_batch_stride, int64_t prior_row_stride, int64_t prior_pixel_stride,
                      const float* weight, int64_t weight_batch_stride, int64_t weight_row_stride,
                      int64_t weight_pixel_stride, int32_t kind, int32_t align, int32_t inverse, float* results,
                      double* stats, void* scratch, int64_t scratch_bytes, void* stream);
int gs_depth_loss_bwd(int64_t batch, int64_t height, int64_t width, const float* depth, int64_t depth_batch_stride,
                      int64_t depth_row_stride, int64_t depth_pixel_stride, const float* prior,
                      int64_t prior_batch_stride, int64_t prior_row_stride, int64_t prior_pixel_stride,
                      const float* weight, int64_t weight_batch_stride, int64_t weight_row_stride,
                      int64_t weight_pixel_stride, int32_t kind, int32_t align, int32_t inverse, const double* stats,
                      const float* g_loss, float* d_depth, void* stream);
int gs_depth_loss_fwd_f64(int64_t batch, int64_t height, int64_t width, const double* depth, int64_t depth_batch_stride,
                          int64_t depth_row_stride, int64_t depth_pixel_stride, const double* prior,
                          int64_t prior_batch_stride, int64_t prior_row_stride, int64_t prior_pixel_stride,
                          const double* weight, int64_t weight_batch_stride, int64_t weight_row_stride,
                          int64_t weight_pixel_stride, int32_t kind, int32_t align, int32_t inverse, double* results,
                          double* stats, void* scratch, int64_t scratch_bytes, void* stream);
int gs_depth_loss_bwd_f64(int64_t batch, int64_t height, int64_t width, const double* depth, int64_t depth_batch_stride,
                          int64_t depth_row_stride, int64_t depth_pixel_stride, const double* prior,
                          int64_t prior_batch_stride, int64_t prior_row_stride, int64_t prior_pixel_stride,
                          const double* weight, int64_t weight_batch_stride, int64_t weight_row_stride,
                          int64_t weight_pixel_stride, int32_t kind, int32_t align, int32_t inverse,
                          const double* stats, const double* g_loss, double* d_depth, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSPLAT_HIP_H */
