// raster_wide.hip -- forward and backward of the alpha blend for feature widths up to GS_MAX_WIDE_FEATURES
// (reference rasterizer/forward.py:25-137 and backward.py:53-228 with a feature size of 64 to 512: features distilled
// from 2D models and lifted to 3D).
//
// The narrow kernels (raster_fwd.hip, raster_bwd.hip) hold a pixel's F channels in registers and blend them inside the
// per-splat walk: at F > 32 that neither fits nor pays.  Here the walk and the channels are separated:
//   * ONE wave64 per 8x8 pixel region, one pixel per lane; splats staged 64 at a time (geometry only) as the narrow
//     kernels' general (MODE 2) records (raster_walk.h), with their per-pixel arithmetic (raster_pdf.h), antialias included.
//   * Forward: the walk records the blend weights w[s][p] = alpha T in LDS; then, per 32-channel chunk of the staged
//     splats' features (LDS), each lane adds sum_s w[s][p] f[s][c] for 4 pixels x 8 channels of the chunk straight
//     into the image (the wave owns its pixels: a load-add-store, no atomics).  Visibility and alpha come from the
//     walk alone.
//   * Backward: the narrow kernel's per-pixel colour state is one scalar, R = sum_c rem_c g_c, and a splat enters a
//     pixel through d = f . g only.  Per batch: D[s][p] = f_s . g_p over all F channels as a 64 x 64 product of LDS
//     chunks (8 splats x 8 pixels per lane); the walk with d = D[s][p] forms the 9 per-splat geometry and heuristic
//     sums (wave butterfly) and overwrites D with the weights; then per chunk, sum_p w[s][p] g_p[c] for 4 splats x 8
//     channels per lane, flushed as 128-byte rows of float atomics.  The heuristics see the full dL/dalpha.
// f32 throughout; the per-(pixel, splat) cost of the walk does not grow with F.

#include "gs_common.h"
#include "raster_pdf.h"
#include "raster_walk.h"

namespace {

constexpr int WC = 32;       // channels per LDS chunk
constexpr int WCP = WC + 4;  // padded chunk row: rows 8 apart fall on distinct banks for the b128 reads
constexpr int WDS = 65;      // row stride of D / w in the backward

struct WideArgs {
  const float* points;
  const float* features;
  const int2* ranges;
  const int* o2p;
  const float* image;       // backward: the forward's image
  const float* grad_image;  // backward
  float* out_image;         // forward
  float* alpha;             // forward
  float* visibility;        // forward, optional
  float* grad_points;       // backward (V,7)
  float* grad_features;     // backward (V,F)
  float* heur;              // backward (V,2), optional
  const float* bg;          // forward, optional: background of channels [bg_off, F) (raster_fwd.hip)
  const float* alpha_in;    // backward, optional: the forward's alpha ...
  const float* grad_weight; // ... and the gradient of the weight image (raster_bwd.hip: R0 = image . g - T g_W)
  int bg_off;
  int W, H, F;
  int tiles_wide, tile_size, side;  // side = tile_size / 8 regions per tile row
  int num_items;
  float cmax, thr, inv_thr, sat_level, tsat, cut;
  int blend, vis, aa, heur_on;
};

// Stage channels [k0, k0 + 32) of 64 rows into an LDS chunk: row r comes from src + row_off(r) (a negative offset
// gives a zero row).  Lane (c = lane & 31, r0 = lane >> 5) loads column c of rows r0, r0 + 2, ...: all 32 loads of a
// lane are issued before the first is waited for (a loop that waits per row exposes one memory latency per row).
template <typename RowOff>
__device__ __forceinline__ void stage_chunk(float (*dst)[WCP], const float* src, int F, int k0, RowOff row_off) {
  const int lane = threadIdx.x, c = lane & 31, r0 = lane >> 5;
  const bool col = k0 + c < F;
  float v[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const int64_t off = row_off(r0 + 2 * i);
    v[i] = (col && off >= 0) ? src[off + k0 + c] : 0.0f;
  }
#pragma unroll
  for (int i = 0; i < 32; ++i) dst[r0 + 2 * i][c] = v[i];
}

__global__ __launch_bounds__(64) void raster_fwd_wide_kernel(const WideArgs a) {
  __shared__ float4 s_geo[64][3];
  __shared__ __attribute__((aligned(16))) float s_w[64][64];  // product weight of staged splat s at pixel p
  __shared__ __attribute__((aligned(16))) float s_f[64][WCP];  // one chunk of the staged splats' features
  __shared__ float s_vis[64];
  __shared__ int s_idx[64];
  int tile, x0, y0;
  if (!gs_wide_region(a, tile, x0, y0)) return;
  const int lane = threadIdx.x;
  const int X = x0 + (lane & 7), Y = y0 + (lane >> 3);
  const bool inb = X < a.W && Y < a.H;
  const float Xf = float(X) + 0.5f, Yf = float(Y) + 0.5f;
  float Tr = inb ? 1.0f : 0.0f;  // forward.py:53-54
  bool done = false;
  // product ownership: pixels 4 pg .. 4 pg + 3 of the region (one pixel row), channels 8 cg .. 8 cg + 7 of a chunk
  const int pg = lane & 15, cg = lane >> 4;
  const int prow = y0 + (pg >> 1), pcol = x0 + (pg & 1) * 4;
  auto out_at = [&](int i) -> float* {
    return (prow < a.H && pcol + i < a.W) ? a.out_image + (int64_t(prow) * a.W + pcol + i) * a.F : nullptr;
  };
  for (int k0 = 0; k0 < a.F; k0 += WC)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (float* o = out_at(i))
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (k0 + 8 * cg + j < a.F) o[k0 + 8 * cg + j] = 0.0f;

  const int2 range_v = a.ranges[tile];
  const int range_x = __builtin_amdgcn_readfirstlane(range_v.x), range_y = __builtin_amdgcn_readfirstlane(range_v.y);
  for (int g0 = range_x; g0 < range_y; g0 += 64) {
    // the early stops of raster_fwd.hip: forward_cut while blending, every pixel done in quantile mode
    const bool open = a.blend ? Tr > a.cut : (inb && !done);
    if (__ballot(open) == 0ull) break;
    const int cnt = __builtin_amdgcn_readfirstlane(min(64, range_y - g0));
    int staged = 0;
    if (lane < cnt) {
      const int idx = a.o2p[g0 + lane];
      const GsSplat sp = gs_load_splat(a.points + int64_t(idx) * 7);
      staged = gs_stage_general<1, false>(s_geo[lane], sp, x0, y0, a.thr, a.inv_thr, a.aa, false);
      s_idx[lane] = idx;
      s_vis[lane] = 0.0f;
    }
    const uint64_t reach = __ballot(staged & 1);
    __syncthreads();  // single-wave workgroup: a wait on the LDS writes
    uint64_t active = 0ull;  // staged splats with a nonzero product weight somewhere in the region
    for (uint64_t m = reach; m != 0ull; m &= m - 1ull) {
      const int j = __builtin_ctzll(m);
      const float4 g0v = s_geo[j][0], g1v = s_geo[j][1], g2v = s_geo[j][2];
      const float alpha = gs_general_alpha(a.aa, Xf - g0v.x, Yf - g0v.y, g0v, g1v, g2v);
      const float al = __builtin_amdgcn_fmed3f(alpha, a.cmax, -1.0f);  // min(alpha, cmax) (forward.py:98-99)
      const bool hit = al > a.thr && !done;
      const float w = (hit ? al : 0.0f) * Tr;
      Tr -= w;
      float pw = a.blend ? w : 0.0f;
      if (!a.blend && hit && 1.0f - Tr >= a.sat_level) {  // forward.py:109-114: the first splat to reach the level
        pw = 1.0f;
        done = true;
      }
      s_w[j][lane] = pw;
      if (__ballot(pw != 0.0f) != 0ull) active |= 1ull << j;
      if (a.vis && __ballot(w != 0.0f) != 0ull) {  // forward.py:116-128
        const float tot = gs_wave_sum_to_lane63(w);
        if (lane == 63) s_vis[j] = tot;
      }
    }
    __syncthreads();
    if (a.vis && lane < cnt && s_vis[lane] != 0.0f) atomicAdd(a.visibility + s_idx[lane], s_vis[lane]);
    if (active == 0ull) continue;  // nothing to blend (the next staging comes after the barrier above)
    for (int k0 = 0; k0 < a.F; k0 += WC) {
      stage_chunk(s_f, a.features, a.F, k0,
                  [&](int s) { return ((active >> s) & 1ull) ? int64_t(s_idx[s]) * a.F : int64_t(-1); });
      __syncthreads();
      float acc[4][8];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.0f;
      for (uint64_t m = active; m != 0ull; m &= m - 1ull) {
        const int s = __builtin_ctzll(m);
        const float4 w4 = *reinterpret_cast<const float4*>(&s_w[s][4 * pg]);
        const float4 fa = *reinterpret_cast<const float4*>(&s_f[s][8 * cg]);
        const float4 fb = *reinterpret_cast<const float4*>(&s_f[s][8 * cg + 4]);
        const float wv[4] = {w4.x, w4.y, w4.z, w4.w}, fv[8] = {fa.x, fa.y, fa.z, fa.w, fb.x, fb.y, fb.z, fb.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[i][j] = __builtin_fmaf(wv[i], fv[j], acc[i][j]);
      }
      // all 32 loads first, from clamped (always valid) addresses, then the guarded stores: a guarded
      // load-add-store per element would wait out one memory latency per element
      float prev[4][8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int px = min(pcol + i, a.W - 1), py = min(prow, a.H - 1);
        const float* o = a.out_image + (int64_t(py) * a.W + px) * a.F;
#pragma unroll
        for (int j = 0; j < 8; ++j) prev[i][j] = o[min(k0 + 8 * cg + j, a.F - 1)];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (float* o = out_at(i))
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (k0 + 8 * cg + j < a.F) o[k0 + 8 * cg + j] = prev[i][j] + acc[i][j];
      __syncthreads();  // s_f is restaged by the next chunk, s_geo / s_w by the next batch
    }
  }
  if (inb) a.alpha[int64_t(Y) * a.W + X] = a.blend ? 1.0f - Tr : (Tr < 1.0f ? 1.0f : 0.0f);  // forward.py:134-137
  if (a.bg != nullptr) {
    // composite on the background: image_c += T bg_c with the transmittance the walk ended with, each lane for the 4
    // pixels x 8 channels per chunk it owns in the product (the wave owns its pixels: a load-add-store as above)
    __syncthreads();  // s_w is free: every batch ends on a barrier, and an empty list never used it
    s_w[0][lane] = Tr;
    __syncthreads();
    const float4 t4 = *reinterpret_cast<const float4*>(&s_w[0][4 * pg]);
    const float tv[4] = {t4.x, t4.y, t4.z, t4.w};
    for (int k0 = 0; k0 < a.F; k0 += WC)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (float* o = out_at(i))
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int c = k0 + 8 * cg + j;
            if (c < a.F && c >= a.bg_off) o[c] = __builtin_fmaf(tv[i], a.bg[c - a.bg_off], o[c]);
          }
  }
}

__global__ __launch_bounds__(64) void raster_bwd_wide_kernel(const WideArgs a) {
  __shared__ float4 s_geo[64][3];
  __shared__ float s_dw[64][WDS];  // D[s][p] = f_s . g_p, overwritten by the walk with the blend weight w[s][p]
  // one chunk of the staged features; then the per-splat sums of the walk; then a chunk of feature gradients
  __shared__ __attribute__((aligned(16))) float s_f[64][WCP];
  __shared__ __attribute__((aligned(16))) float s_g[64][WCP];  // one chunk of the region's pixel gradients
  __shared__ int s_idx[64];
  float(*s_acc)[9] = reinterpret_cast<float(*)[9]>(&s_f[0][0]);
  int tile, x0, y0;
  if (!gs_wide_region(a, tile, x0, y0)) return;
  const int lane = threadIdx.x;
  const int X = x0 + (lane & 7), Y = y0 + (lane >> 3);
  const bool inb = X < a.W && Y < a.H;
  const float Xf = float(X) + 0.5f, Yf = float(Y) + 0.5f;
  float Tr = inb ? 1.0f : 0.0f;  // backward.py:99-112
  float R = 0.0f;                // sum_c image_c g_c: the remaining colour dotted with the pixel's gradient
  const int my_slot = (lane & 3) == 0 ? gs_reduce_slot<9>(lane) : (lane == 60 ? 8 : -1);
  const int sb = lane & 7, pb = lane >> 3;  // D ownership: splats sb + 8 i, pixels pb + 8 j
  const int sg = lane & 15, cg = lane >> 4;  // feature-gradient ownership: splats sg + 16 i, channels 8 cg .. 8 cg + 7
  const int W = a.W, H = a.H, F = a.F;
  auto pixel_row = [=](int p) {
    const int px = x0 + (p & 7), py = y0 + (p >> 3);
    return (px < W && py < H) ? (int64_t(py) * W + px) * F : int64_t(-1);
  };
  const float* grad_image = a.grad_image;
  auto stage_g = [&](int k0) { stage_chunk(s_g, grad_image, F, k0, pixel_row); };

  for (int k0 = 0; k0 < a.F; k0 += WC) {  // R = image . g, one chunk of both images at a time
    stage_g(k0);
    stage_chunk(s_f, a.image, a.F, k0, pixel_row);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < WC; c += 4) {
      const float4 u = *reinterpret_cast<const float4*>(&s_f[lane][c]);
      const float4 g = *reinterpret_cast<const float4*>(&s_g[lane][c]);
      R = __builtin_fmaf(u.x, g.x, __builtin_fmaf(u.y, g.y, __builtin_fmaf(u.z, g.z, __builtin_fmaf(u.w, g.w, R))));
    }
    __syncthreads();
  }
  if (a.grad_weight != nullptr && inb) {
    const int64_t pix = int64_t(Y) * a.W + X;
    R = __builtin_fmaf(a.alpha_in[pix] - 1.0f, a.grad_weight[pix], R);
  }

  const int2 range_v = a.ranges[tile];
  const int range_x = __builtin_amdgcn_readfirstlane(range_v.x), range_y = __builtin_amdgcn_readfirstlane(range_v.y);
  for (int g0 = range_x; g0 < range_y; g0 += 64) {
    if (__ballot(Tr > a.tsat) == 0ull) break;  // every pixel saturated (backward.py:116-118)
    const int cnt = __builtin_amdgcn_readfirstlane(min(64, range_y - g0));
    int staged = 0;
    if (lane < cnt) {
      const int idx = a.o2p[g0 + lane];
      const GsSplat sp = gs_load_splat(a.points + int64_t(idx) * 7);
      staged = gs_stage_general<1, true>(s_geo[lane], sp, x0, y0, a.thr, a.inv_thr, a.aa, false);
      s_idx[lane] = idx;
    }
    const uint64_t reach = __ballot(staged & 1);
    __syncthreads();
    if (reach == 0ull) continue;  // no staged splat reaches the region

    // ---- D[s][p] = f_s . g_p over all channels
    float D[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) D[i][j] = 0.0f;
    for (int k0 = 0; k0 < a.F; k0 += WC) {
      stage_chunk(s_f, a.features, a.F, k0,
                  [&](int s) { return ((reach >> s) & 1ull) ? int64_t(s_idx[s]) * a.F : int64_t(-1); });
      stage_g(k0);
      __syncthreads();
#pragma unroll 1
      for (int c = 0; c < WC; c += 4) {
        float4 fv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) fv[i] = *reinterpret_cast<const float4*>(&s_f[sb + 8 * i][c]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float4 gv = *reinterpret_cast<const float4*>(&s_g[pb + 8 * j][c]);
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            float d = D[i][j];
            d = __builtin_fmaf(fv[i].x, gv.x, d);
            d = __builtin_fmaf(fv[i].y, gv.y, d);
            d = __builtin_fmaf(fv[i].z, gv.z, d);
            D[i][j] = __builtin_fmaf(fv[i].w, gv.w, d);
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) s_dw[sb + 8 * i][pb + 8 * j] = D[i][j];
#pragma unroll
    for (int c = 0; c < 9; ++c) s_acc[lane][c] = 0.0f;
    __syncthreads();

    // ---- the walk (the narrow MODE 2 arithmetic, raster_pdf.h, with d = D[s][p] for f . g); D[j][p] becomes w[j][p]
    for (int j = 0; j < cnt; ++j) {
      if (!((reach >> j) & 1ull)) {
        s_dw[j][lane] = 0.0f;
        continue;
      }
      const float d = s_dw[j][lane];
      const float4 g0v = s_geo[j][0], g1v = s_geo[j][1], g2v = s_geo[j][2];
      const float dx = Xf - g0v.x, dy = Yf - g0v.y;
      float p, dmx = 0, dmy = 0, dax = 0, day = 0, dsx = 0, dsy = 0, Px = 0, Py = 0;
      float aa_z[4] = {0, 0, 0, 0}, aa_a[4] = {0, 0, 0, 0};
      if (a.aa) {
        // the antialiased pdf's value half, written out as in raster_bwd.hip (raster_pdf.h says why, and what it is)
        const float ux = dx * g2v.x + dy * g2v.y, uy = dy * g2v.x - dx * g2v.y;
        aa_z[0] = __builtin_fmaf(ux, g2v.z, g1v.x); aa_z[1] = __builtin_fmaf(ux, g2v.z, -g1v.x);
        aa_z[2] = __builtin_fmaf(uy, g2v.w, g1v.y); aa_z[3] = __builtin_fmaf(uy, g2v.w, -g1v.y);
#pragma unroll
        for (int k = 0; k < 4; ++k) aa_a[k] = s_sig_value(aa_z[k]);
        p = 6.28318530717958648f * (g0v.z * (aa_a[0] - aa_a[1])) * (g0v.w * (aa_a[2] - aa_a[3]));
      } else {
        float tx, ty;
        p = gs_general_pdf_plain(dx, dy, g0v, g1v, g2v, tx, ty, dmx, dmy, dax, day, dsx, dsy);
      }
      const float alpha_raw = g1v.z * p;
      const bool hit = alpha_raw > a.thr && Tr > a.tsat;  // backward.py:160,166
      float v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      float w = 0.0f;
      if (hit) {
        if (a.aa) gs_general_pdf_gradient(dx, dy, g0v, aa_z, aa_a, Px, Py, dax, day, dsx, dsy);
        const float alc = __builtin_amdgcn_fmed3f(alpha_raw, a.cmax, -1.0f);  // min(alpha, cmax) (:169)
        w = alc * Tr;
        // dL/dalpha = (T d - R) / (1 - alpha), R still including this splat's share (:180-182)
        const float alpha_grad = (Tr * d - R) * gs_rcp_fast(1.0f - alc);
        gs_general_sums<false>(a.aa, 1, g1v, g2v, p, dmx, dmy, dax, day, dsx, dsy, Px, Py, alpha_grad, v);
        Tr = __builtin_fmaf(-Tr, alc, Tr);
        R = __builtin_fmaf(-d, w, R);
      }
      s_dw[j][lane] = w;
      if (__ballot(hit) != 0ull) {
        const float tot = gs_wave_reduce_transposed<9>(v, lane);
        if (my_slot >= 0) s_acc[j][my_slot] = tot;
      }
    }
    __syncthreads();

    // ---- per-splat geometry gradients and heuristics: lane j, splat j
    if (lane < cnt && ((reach >> lane) & 1ull)) {
      float t[9];
#pragma unroll
      for (int c = 0; c < 9; ++c) t[c] = s_acc[lane][c];
      if (a.aa) {  // the mean's gradient out of the splat frame
        const float ax = s_geo[lane][2].x, ay = s_geo[lane][2].y;
        gs_mean_grad_from_splat_frame(t[0], t[1], ax, ay);
      }
      const int64_t idx = s_idx[lane];
#pragma unroll
      for (int c = 0; c < 7; ++c)
        if (t[c] != 0.0f) atomicAdd(a.grad_points + idx * 7 + c, t[c]);
      if (a.heur_on && a.heur) {
        if (t[7] != 0.0f) atomicAdd(a.heur + idx * 2, t[7]);
        if (t[8] != 0.0f) atomicAdd(a.heur + idx * 2 + 1, t[8]);
      }
    }
    __syncthreads();  // s_acc (in s_f) is read; s_f now takes the feature gradients

    // ---- feature gradients sum_p w[s][p] g_p, one 32-channel chunk at a time
    for (int k0 = 0; k0 < a.F; k0 += WC) {
      stage_g(k0);
      __syncthreads();
      float acc[4][8];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.0f;
#pragma unroll 4
      for (int p = 0; p < 64; ++p) {
        const float4 ga = *reinterpret_cast<const float4*>(&s_g[p][8 * cg]);
        const float4 gb = *reinterpret_cast<const float4*>(&s_g[p][8 * cg + 4]);
        const float gv[8] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y, gb.z, gb.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float wv = s_dw[sg + 16 * i][p];
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[i][j] = __builtin_fmaf(wv, gv[j], acc[i][j]);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) s_f[sg + 16 * i][8 * cg + j] = acc[i][j];
      __syncthreads();
      // flush: a wave atomic instruction covers two splats' 32 contiguous channels (128 bytes each)
      for (int e = lane; e < cnt * WC; e += 64) {
        const int s = e / WC, c = e - s * WC;
        const float val = s_f[s][c];
        if (k0 + c < a.F && val != 0.0f) atomicAdd(a.grad_features + int64_t(s_idx[s]) * a.F + k0 + c, val);
      }
      __syncthreads();
    }
  }
}

int wide_setup(const char* what, int32_t num_features, int32_t width, int32_t height, const GsRasterConfig* cfg,
               WideArgs& a) {
  if (int rc = gs_check_cfg(cfg)) return rc;
  if (int rc = gs_check_raster_call(what, width, height, num_features, GS_MAX_WIDE_FEATURES)) return rc;
  a = WideArgs{};
  const int ts = cfg->tile_size;
  a.W = width; a.H = height; a.F = num_features;
  a.tiles_wide = int(gs_div_up(width, ts));
  a.tile_size = ts;
  a.side = ts / 8;
  a.num_items = int(a.tiles_wide * gs_div_up(height, ts) * a.side * a.side);
  a.cmax = cfg->clamp_max_alpha; a.thr = cfg->alpha_threshold; a.inv_thr = 1.0f / cfg->alpha_threshold;
  a.sat_level = 1.0f - cfg->saturate_threshold;
  a.tsat = 1.0f - cfg->saturate_threshold;
  a.cut = gs_forward_cut(cfg);
  a.blend = cfg->use_alpha_blending; a.aa = cfg->antialias;
  a.vis = cfg->compute_visibility || cfg->compute_point_heuristic;
  a.heur_on = cfg->compute_point_heuristic;
  return GS_OK;
}

}  // namespace

extern "C" int gs_raster_fwd_wide(int64_t v, int32_t num_features, const float* points, const float* features,
                                  const int32_t* tile_ranges, const int32_t* overlap_to_point, int64_t k, int32_t width,
                                  int32_t height, const GsRasterConfig* cfg, float* image, float* alpha,
                                  float* visibility, const float* background, int32_t background_offset,
                                  void* stream) {
  WideArgs a;
  if (int rc = wide_setup("gs_raster_fwd_wide", num_features, width, height, cfg, a)) return rc;
  if (int rc = gs_check_background("gs_raster_fwd_wide", cfg->use_alpha_blending, background != nullptr,
                                   background_offset, num_features))
    return rc;
  a.bg = background; a.bg_off = background ? background_offset : 0;
  if (int rc = gs_check_raster_fwd_buffers("gs_raster_fwd_wide", image, alpha, tile_ranges, k, points, features,
                                           overlap_to_point, a.vis != 0, visibility, v))
    return rc;
  a.points = points; a.features = features; a.ranges = reinterpret_cast<const int2*>(tile_ranges);
  a.o2p = overlap_to_point; a.out_image = image; a.alpha = alpha; a.visibility = visibility;
  if (v == 0) a.vis = 0;
  hipLaunchKernelGGL(raster_fwd_wide_kernel, dim3(unsigned(8 * gs_div_up(a.num_items, 8))), dim3(64), 0,
                     static_cast<hipStream_t>(stream), a);
  GS_CHECK_LAUNCH("gs_raster_fwd_wide");
  return GS_OK;
}

extern "C" int gs_raster_bwd_wide(int64_t v, int32_t num_features, const float* points, const float* features,
                                  const int32_t* tile_ranges, const int32_t* overlap_to_point, int64_t k, int32_t width,
                                  int32_t height, const GsRasterConfig* cfg, const float* image,
                                  const float* grad_image, const float* alpha, const float* grad_weight,
                                  float* grad_points, float* grad_features, float* point_heuristic, void* stream) {
  WideArgs a;
  if (int rc = wide_setup("gs_raster_bwd_wide", num_features, width, height, cfg, a)) return rc;
  GS_REQUIRE(!grad_weight || alpha, GS_ERR_INVALID_ARGUMENT,
             "gs_raster_bwd_wide: grad_weight without the forward's alpha image");
  a.alpha_in = alpha; a.grad_weight = grad_weight;
  GS_REQUIRE(cfg->use_alpha_blending, GS_ERR_UNSUPPORTED,
             "gs_raster_bwd_wide: no gradient is defined without alpha blending");
  GS_REQUIRE(image && grad_image && tile_ranges, GS_ERR_INVALID_ARGUMENT, "gs_raster_bwd_wide: NULL image or ranges");
  if (k == 0 || v == 0) return GS_OK;
  GS_REQUIRE(points && features && overlap_to_point && grad_points && grad_features, GS_ERR_INVALID_ARGUMENT,
             "gs_raster_bwd_wide: NULL input or gradient output");
  GS_REQUIRE(!a.heur_on || point_heuristic, GS_ERR_INVALID_ARGUMENT, "gs_raster_bwd_wide: point_heuristic is NULL");
  a.points = points; a.features = features; a.ranges = reinterpret_cast<const int2*>(tile_ranges);
  a.o2p = overlap_to_point; a.image = image; a.grad_image = grad_image;
  a.grad_points = grad_points; a.grad_features = grad_features; a.heur = point_heuristic;
  hipLaunchKernelGGL(raster_bwd_wide_kernel, dim3(unsigned(8 * gs_div_up(a.num_items, 8))), dim3(64), 0,
                     static_cast<hipStream_t>(stream), a);
  GS_CHECK_LAUNCH("gs_raster_bwd_wide");
  return GS_OK;
}
