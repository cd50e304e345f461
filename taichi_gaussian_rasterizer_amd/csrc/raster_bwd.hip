// raster_bwd.hip -- gradient backward of the alpha-blend (reference rasterizer/backward.py:53-228,
// pdf gradients taichi_lib/generic.py:321-336 / :371-404).
//
// Same wave-per-16x16-region layout, LDS staging and scalar sub-block masks as raster_fwd.hip, from the same code
// (raster_walk.h); MODE 2's plain pdf, pdf gradients and per-pixel sums are raster_pdf.h, shared with raster_wide.hip.
// What is specific to the backward:
//   * Front-to-back re-traversal with the FINAL image as the "remaining colour"
//     (backward.py:110,177-180).  The remaining colour only ever appears dotted with the pixel's
//     upstream gradient, so each pixel carries ONE scalar R = sum_c rem_c * g_c instead of F
//     channels:  R -= w * (f . g);  dL/dalpha = T (f . g) - R / (1 - alpha).
//   * Lean kernel: the pdf gradients are linear in a few per-pixel moments, so each lane
//     accumulates 6 sums in the ellipse frame (G, G tx, G ty, G tx^2, G tx ty, G ty^2 with
//     G = p * dL/dalpha; tx, ty are O(1) so nothing cancels) + F feature sums over its <= 4 pixels;
//     the 7 splat gradients are formed from the wave totals once per splat, 64 splats at a time
//     (one lane per splat).
//   * Wave reduction by fused v_add_f32_dpp (row_ror 8/4/2/1, row_bcast 15/31): a workgroup is
//     exactly one wave64, so the whole-tile reduction needs no LDS atomics and no barrier
//     (the reference: warp shuffle -> shared atomic -> global atomic, concurrent.py:81-85).
//   * Flush: one 64-byte-aligned row per Gaussian in grad_rows; a wave atomic instruction
//     covers 4 splats x 16 contiguous floats (four 64-B memory-side atomic requests) instead of 64
//     scattered dwords -- the difference between ~1.3 TB/s and ~0.08 TB/s of atomic bytes on
//     MI355X (MI355X_MICROARCH.md, Global float atomics).
//
// Roofline: algorithmic HBM bytes 8T + K(4+28+4F) + 8PF + 4(7+F)K; VALU-bound.

#include "gs_common.h"
#include "raster_pdf.h"
#include "raster_walk.h"

namespace {

struct BwdArgs {
  const float* points;
  const float* features;
  const int2* ranges;
  const int* o2p;
  const float* image;
  const float* grad_image;
  float* grad_rows;
  int W, H, F;
  int row_floats;
  int tiles_wide;
  int tile_size;
  int sub_x, sub_y;  // wave regions per tile along x / y
  int num_items;
  int num_tiles;
  const int* heavy;  // optional (device): the first *heavy entries of tile_order get four 8x8 workgroups each
  int heavy_cap;
  const int* tile_order;  // optional launch order of the items (heaviest first)
  float cmax, thr, inv_thr, sat;
  int aa, heur;
  GsShard sh;  // owned tile rows: tile ids are local, H is the full image height, the images hold the owned rows
  // optional gradient of the weight image: dT/dalpha_i = -T / (1 - alpha_i) for the final transmittance T = 1 - weight,
  // so dL/dweight enters as one more term of each pixel's INITIAL R, R0 = image . g - T g_W (image: the forward's,
  // background included, which carries the background's own T bg . g).  Both NULL = the weight is a constant.
  const float* alpha;
  const float* grad_weight;
};

// LDS arena of one wave: sized by the 64-splat staging group, not by the wave's pixel region
// MODE 0: lean (6 ellipse-frame moments); 1: lean + the two densification heuristics (training with statistics);
// 2: full (7 gradients + 2 heuristics per pixel; antialiased pdf)
template <int FP, int MODE>
struct BwdShape {
  static constexpr bool FULL = MODE == 2;
  static constexpr int NS = MODE == 2 ? 9 : MODE == 1 ? 8 : 6;  // sums per splat besides the F feature gradients
  static constexpr int NACC = NS + FP;           // values reduced per splat
  static constexpr int ROW = ((9 + FP + 15) / 16) * 16;
  static constexpr int GEO_V4 = FULL ? 3 : 2;     // float4s of geometry per staged record ...
  static constexpr int REC_V4 = GEO_V4 + (FP + 3) / 4;  // ... followed by the feature row: one address, b128 reads
  // the per-splat totals are read back one lane per splat, so any ODD stride is conflict-free
  static constexpr int REC_F = 64 * 4 * REC_V4, ACC_STRIDE = NACC | 1, ACC_F = 64 * ACC_STRIDE;
  static constexpr int OUT_STRIDE = ROW + 1, OUT_F = 64 * OUT_STRIDE;
  static constexpr int ARENA_F = (REC_F + ACC_F) > OUT_F ? (REC_F + ACC_F) : OUT_F;
};

// How a wave walks one staged splat.  The kernel is bound by VALU issue, so each step hands what it can to a unit that
// has time; what was measured against each choice is recorded in DESIGN 4 and profiles/r3/.
//   * The per-splat sums start as zeros READ FROM LDS: ceil(NACC / 4) ds_read_b128 of a 64-byte block of zeros at the
//     head of every splat, their latency under the first sub-block's coordinate / exponent arithmetic, and every
//     sub-block accumulates.  (Kernels with up to 16 sums per splat.  Lost: `= 0.0f`, which costs nine v_mov_b32 whenever
//     the first sub-block is masked out -- profiles/r3/ab_zero_sums_from_lds.txt.)
//   * The sub-block masks of the staged splats are four 64-bit ballots in scalar registers (bit j of ballot b: splat j
//     reaches sub-block b, and b is still live): the walk tests them with scalar bit tests only, and its branches do
//     not wait for the splat's LDS record.  (Lost: the mask as a word of the record, made scalar with a
//     v_readfirstlane per splat -- profiles/r3/ab_mask_ballots_bwd.txt.)
//   * The next splat's record is fetched in front of the wave reduction, into the registers of the record just used.
//     (Lost: the fetch at the head of the iteration -- profiles/r3/ab_fetch_ahead.txt.)
//   * Everything behind the hit test runs under EXEC = the pixels that take something from the splat; nobody adds
//     zeros.  (Lost: a select that zeroed alpha for the other pixels, and a wave-level "nobody hit" branch in front --
//     profiles/r3/ab_hit_under_exec.txt, ab_hit_exec_no_wave_branch.txt.)
//   * The wave sum is the transposed register butterfly (gs_common.h).  Of nine sums (lean, F = 3) the ninth does not
//     fit the 8-value butterfly: four DPP adds leave every lane with its ROW's sum, and one lane per row adds that to
//     the splat's total in LDS (ds_add_f32, four lanes on one address; the Makefile keeps it one instruction).  (Lost:
//     six DPP adds to row 3 -- ab_ninth_value_lds_add.txt; the reduction transposed through LDS in one, two or half a
//     pass -- ubench_mfma_reduce.txt, kernel_table_lds_reduce_v2.txt, ab_hybrid_reduce.txt; the butterfly ending in a
//     32-lane ds_add_f32 -- ab_butterfly_quarter_lds_add.txt; its swap stages through the LDS crossbar -- the last
//     "not kept" entry of that list in DESIGN 4.)
template <int NB, int FP, int MODE>
__device__ __forceinline__ void raster_bwd_body(const BwdArgs& a, int tile, int x0, int y0, int yout0, float* smem,
                                                const float* s_zeros) {
  const int lane = threadIdx.x;
  constexpr bool FULL = MODE == 2, HEUR = MODE == 1;

  // One LDS arena per wave.  The staged records (geo, feat) and the per-splat totals (acc) are dead
  // by the time the gradient rows (out) are written, so `out` aliases them: ~7.4 KB per wave
  // instead of ~11.5 KB, i.e. 21 instead of 13 resident waves per CU.
  typedef BwdShape<FP, MODE> Shape;
  constexpr int NS = Shape::NS, NACC = Shape::NACC, ROW = Shape::ROW;
  constexpr int GEO_V4 = Shape::GEO_V4, REC_V4 = Shape::REC_V4, ACC_STRIDE = Shape::ACC_STRIDE;
  constexpr int OUT_STRIDE = Shape::OUT_STRIDE;
  float4(*s_geo)[REC_V4] = reinterpret_cast<float4(*)[REC_V4]>(smem);
  float(*s_acc)[ACC_STRIDE] = reinterpret_cast<float(*)[ACC_STRIDE]>(smem + Shape::REC_F);
  float(*s_out)[OUT_STRIDE] = reinterpret_cast<float(*)[OUT_STRIDE]>(smem);

  // which value of the per-splat reduction this lane ends up owning (lane-constant; -1 = none)
  constexpr bool NINTH_LDS = NACC == 9;
  constexpr int NBUTTERFLY = NINTH_LDS ? 8 : (NACC <= 16 ? NACC : 1);
  const int my_slot = (NACC <= 16 && (lane & 3) == 0) ? gs_reduce_slot<NBUTTERFLY>(lane) : -1;
  const int lx = lane & 7, ly = lane >> 3;
  // Tr = 1 - (accumulated weight): the transmittance in front of the next splat.  The reference carries the weight W
  // and tests W < saturate_threshold (backward.py:160); Tr > 1 - saturate_threshold is the same test, and every use of
  // W in the gradient is through 1 - W.
  const float tsat = 1.0f - a.sat;
  float Xf[NB], Yf[NB], Tr[NB], R[NB], gpix[NB][FP];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int X = x0 + (b & 1) * 8 + lx, Y = y0 + (b >> 1) * 8 + ly;
    const bool inb = X < a.W && Y < a.H;
    // lean modes: pixel centres relative to the wave's origin, as in the forward (raster_fwd.hip)
    Xf[b] = FULL ? float(X) + 0.5f : float((b & 1) * 8 + lx) + 0.5f;
    Yf[b] = FULL ? float(Y) + 0.5f : float((b >> 1) * 8 + ly) + 0.5f;
    Tr[b] = inb ? 1.0f : 0.0f;  // backward.py:99-112: out-of-image pixels start saturated
    R[b] = 0.0f;
#pragma unroll
    for (int c = 0; c < FP; ++c) gpix[b][c] = 0.0f;
    if (inb) {
      const int64_t pix = int64_t(Y - y0 + yout0) * a.W + X;
#pragma unroll
      for (int c = 0; c < FP; ++c)
        if (c < a.F) {
          gpix[b][c] = a.grad_image[pix * a.F + c];
          R[b] += a.image[pix * a.F + c] * gpix[b][c];
        }
    }
  }
  if (a.grad_weight != nullptr) {  // wave-uniform (a kernel argument); nothing inside the splat loop changes
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int X = x0 + (b & 1) * 8 + lx, Y = y0 + (b >> 1) * 8 + ly;
      if (X < a.W && Y < a.H) {
        const int64_t pix = int64_t(Y - y0 + yout0) * a.W + X;
        R[b] = __builtin_fmaf(a.alpha[pix] - 1.0f, a.grad_weight[pix], R[b]);
      }
    }
  }

  const int2 range_v = a.ranges[tile];
  // wave-uniform: keep the loop bounds in scalar registers
  const int range_x = __builtin_amdgcn_readfirstlane(range_v.x), range_y = __builtin_amdgcn_readfirstlane(range_v.y);
  // lean kernels stage the ellipse frame scaled by K_EXP so that the pdf is exp2(-(tx^2 + ty^2)) with no further
  // multiply; the moments are accumulated in those coordinates and unscaled once per splat in the epilogue
  constexpr float IK = 1.0f / GS_K_EXP, IK2 = IK * IK;

  int zero_off = 0;  // byte offset of the zeros read at the head of every splat (see above)
  for (int g0 = range_x; g0 < range_y; g0 += 64) {
    // all pixels of the region saturated -> nothing further contributes (backward.py:116-118)
    // ... and a saturated 8x8 sub-block takes no gradient from here on (:160,166): masked out before its alphas
    // are even computed
    int live = 0;
#pragma unroll
    for (int b = 0; b < NB; ++b)
      if (__ballot(Tr[b] > tsat) != 0ull) live |= 1 << b;
    if (live == 0) break;

    const int cnt = __builtin_amdgcn_readfirstlane(min(64, range_y - g0));
    float ax = 0, ay = 0, isx = 0, isy = 0, al = 0;
    int idx = 0;
    int staged_mask = 0;
    if (lane < cnt) {
      idx = a.o2p[g0 + lane];
      const GsSplat sp = gs_load_splat(a.points + int64_t(idx) * 7);
      ax = sp.ax; ay = sp.ay; isx = sp.isx; isy = sp.isy; al = sp.al;
      // the record's geometry and the conservative sub-block mask: the forward's own expressions (raster_walk.h), so a
      // pixel is hit here exactly when it was there
      staged_mask = FULL ? gs_stage_general<NB, true>(s_geo[lane], sp, x0, y0, a.thr, a.inv_thr, a.aa, true)
                         : gs_stage_lean<NB>(s_geo[lane], sp, x0, y0, a.thr, a.inv_thr);
      gs_stage_features<FP, GEO_V4>(s_geo[lane], a.features + int64_t(idx) * a.F, a.F);
    }
#pragma unroll
    for (int c = 0; c < NACC; ++c) s_acc[lane][c] = 0.0f;
    __syncthreads();

    float4 g0v, g1v, g2v = make_float4(0, 0, 0, 0);
    float feat[FP];
    auto fetch_record = [&](int j) {
      g0v = s_geo[j][0];
      g1v = s_geo[j][1];
      if (FULL) g2v = s_geo[j][2];
      gs_fetch_features<FP, GEO_V4>(s_geo[j], feat);
    };
    fetch_record(0);
    uint64_t reach[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
      reach[b] = ((live >> b) & 1) ? __ballot((staged_mask >> b) & 1) : 0ull;
    for (int j = 0; j < cnt; ++j) {
      int mask = 0;
#pragma unroll
      for (int b = 0; b < NB; ++b) mask |= int((reach[b] >> j) & 1ull) << b;

      float S[NS], gf[FP];
      if (NACC <= 16) {
        // (an opaque byte OFFSET, carried across the loop: an opaque pointer would lose its address space and become a
        // flat load; re-initialising it per splat would cost the v_mov this is about)
        asm volatile("" : "+v"(zero_off));
        const float4* zp = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_zeros) + zero_off);
        float z[16];
#pragma unroll
        for (int q = 0; q < (NACC + 3) / 4; ++q) {
          const float4 zq = zp[q];
          z[4 * q] = zq.x; z[4 * q + 1] = zq.y; z[4 * q + 2] = zq.z; z[4 * q + 3] = zq.w;
        }
#pragma unroll
        for (int c = 0; c < NS; ++c) S[c] = z[c];
#pragma unroll
        for (int c = 0; c < FP; ++c) gf[c] = z[(NS + c) < 16 ? NS + c : 0];
      } else {
#pragma unroll
        for (int c = 0; c < NS; ++c) S[c] = 0.0f;
#pragma unroll
        for (int c = 0; c < FP; ++c) gf[c] = 0.0f;
      }
      uint64_t hit_lanes = 0ull;  // the pixels, of any sub-block, that took a gradient from this splat

#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (!(mask & (1 << b))) continue;  // scalar branch
        const float dx = FULL ? Xf[b] - g0v.x : 0.0f, dy = FULL ? Yf[b] - g0v.y : 0.0f;
        float p, tx = 0, ty = 0;
        float dmx = 0, dmy = 0, dax = 0, day = 0, dsx = 0, dsy = 0;
        float Px = 0, Py = 0;  // antialias: d pdf / d (ux, uy), the splat-frame gradient the mean and axis terms share
        float aa_z[4] = {0, 0, 0, 0}, aa_a[4] = {0, 0, 0, 0};  // antialias: sigmoid arguments and values
        // (the antialiased pdf's value half stays written out, here and in raster_wide.hip: as a call these kernels take
        // more registers; the rest of the general mode is raster_pdf.h, where the formulas and the record's layout are)
        if (FULL && a.aa) {
          const float ux = dx * g2v.x + dy * g2v.y, uy = dy * g2v.x - dx * g2v.y;
          aa_z[0] = __builtin_fmaf(ux, g2v.z, g1v.x); aa_z[1] = __builtin_fmaf(ux, g2v.z, -g1v.x);
          aa_z[2] = __builtin_fmaf(uy, g2v.w, g1v.y); aa_z[3] = __builtin_fmaf(uy, g2v.w, -g1v.y);
#pragma unroll
          for (int k = 0; k < 4; ++k) aa_a[k] = s_sig_value(aa_z[k]);
          p = 6.28318530717958648f * (g0v.z * (aa_a[0] - aa_a[1])) * (g0v.w * (aa_a[2] - aa_a[3]));
        } else if (FULL) {
          p = gs_general_pdf_plain(dx, dy, g0v, g1v, g2v, tx, ty, dmx, dmy, dax, day, dsx, dsy);
        } else {
          tx = __builtin_fmaf(g0v.z, Xf[b], __builtin_fmaf(g0v.w, Yf[b], g0v.x));
          ty = __builtin_fmaf(g1v.x, Xf[b], __builtin_fmaf(g1v.y, Yf[b], g0v.y));
          // the record carries -log2(opacity), p is alpha itself (same expression as the forward: same bits)
          p = gs_exp2_fast(-__builtin_fmaf(ty, ty, __builtin_fmaf(tx, tx, g1v.z)));
        }
        const float alpha_raw = FULL ? g1v.z * p : p;
        const bool over = alpha_raw > a.thr, open = Tr[b] > tsat;
        const bool hit = over && open;  // backward.py:160,166
        // (two ballots of plain compares and a scalar AND: a ballot of the conjunction is rebuilt through a VGPR)
        hit_lanes |= __ballot(over) & __ballot(open);  // scalar; the EXEC-masked block below skips itself when empty
        // Everything below is linear in the pixel's alpha and touches nothing but the lane's own sums and state: it runs
        // under EXEC = the pixels that take something from this splat (a partly empty EXEC costs a wave64 instruction
        // nothing extra), so nobody has to zero alpha for the others.
        if (!hit) continue;
        if (FULL && a.aa) gs_general_pdf_gradient(dx, dy, g0v, aa_z, aa_a, Px, Py, dax, day, dsx, dsy);
        const float alc = __builtin_amdgcn_fmed3f(alpha_raw, a.cmax, -1.0f);  // min(alpha, cmax), one v_med3_f32 (:169)
        float dot = 0.0f;
#pragma unroll
        for (int c = 0; c < FP; ++c) dot += feat[c] * gpix[b][c];
        // dL/dalpha = sum_c (f_c T - rem_c / (1 - alpha)) g_c   (:180-182) with rem = R - w dot, w = alpha T:
        //           = (T dot - R) / (1 - alpha), R still including this splat's share.  The numerator is formed before
        // T and R are updated so that both updates happen in place (no register copies at the end of the block).
        const float num = Tr[b] * dot - R[b];
        const float w = alc * Tr[b];
        const float alpha_grad = num * gs_rcp_fast(1.0f - alc);
#pragma unroll
        for (int c = 0; c < FP; ++c) gf[c] += w * gpix[b][c];  // :201
        if (FULL) {
          gs_general_sums<true>(a.aa, a.heur, g1v, g2v, p, dmx, dmy, dax, day, dsx, dsy, Px, Py, alpha_grad, S);
        } else {
          // moments in the (scaled) ellipse frame (tx, ty are O(1): no cancellation for elongated splats), carrying
          // the splat's opacity: G = alpha_p * pdf * dL/dalpha
          const float G = alpha_raw * alpha_grad;
          const float Gtx = G * tx, Gty = G * ty;
          S[0] += G;
          S[1] += Gtx; S[2] += Gty;
          S[3] += Gtx * tx; S[4] += Gtx * ty; S[5] += Gty * ty;
          if (HEUR) {
            // backward.py:194-198 from the lean record: dp/dmean = p (tx A + ty B), A = axis / sx, B = perp(axis) / sy
            S[6] += alpha_grad * alpha_grad;  // hit-masked in this mode; the epilogue applies alpha_p^2
            // |alpha_p dL/dalpha dp/dmean|_1 = |G| (|tx A.x + ty B.x| + |tx A.y + ty B.y|) / K_EXP^2 with
            // G = alpha_p pdf dL/dalpha as above (the staged frame and tx, ty both carry K_EXP; the constant is
            // applied once per splat in the epilogue)
            S[7] += fabsf(G) * (fabsf(tx * g0v.z + ty * g1v.x) + fabsf(tx * g0v.w + ty * g1v.y));
          }
        }
        // T -= alpha T and R -= w dot, last and in place: left to the scheduler, the new values are formed early in
        // temporaries (the old ones are still needed for `num`) and copied back with two v_mov_b32 per block
        asm("v_fma_f32 %0, -%0, %1, %0" : "+v"(Tr[b]) : "v"(alc));
        asm("v_fma_f32 %0, -%1, %2, %0" : "+v"(R[b]) : "v"(dot), "v"(w));
      }

      // The record's registers are dead from here to the end of the iteration: the next splat's record is fetched into
      // them NOW, so that its LDS latency passes under the reduction below instead of in front of the next splat's
      // first instruction (no second register set, no copies).
      fetch_record(min(j + 1, 63));
      // reduce over the wave only if some pixel took a gradient (backward.py:204)
      if (hit_lanes != 0ull) {
        // transposed butterfly over the wave, sized for the exact number of values; the lane that ends
        // up owning value k stores it (one ds_write_b32 for all values of a chunk)
        if (NINTH_LDS) {
          float w8[8];
#pragma unroll
          for (int c = 0; c < 8; ++c) w8[c] = c < NS ? S[c < NS ? c : 0] : gf[c >= NS ? c - NS : 0];
          float x = gf[FP - 1];  // value 8
          x = gs_dpp_add_full<0x128>(x);  // row_ror:8
          x = gs_dpp_add_full<0x124>(x);  // row_ror:4
          x = gs_dpp_add_full<0x122>(x);  // row_ror:2
          x = gs_dpp_add_full<0x121>(x);  // row_ror:1 -> every lane holds its row's sum
          const float tot = gs_wave_reduce_transposed<8>(w8, lane);
          if (my_slot >= 0) s_acc[j][my_slot] = tot;
          if ((lane & 15) == 0)
            __hip_atomic_fetch_add(&s_acc[j][8], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // 0 at staging
        } else if (NACC <= 16) {
          float vals[NACC <= 16 ? NACC : 1];
#pragma unroll
          for (int c = 0; c < NACC && c < 16; ++c) vals[c] = c < NS ? S[c < NS ? c : 0] : gf[c >= NS ? c - NS : 0];
          const float tot = gs_wave_reduce_transposed<(NACC <= 16 ? NACC : 1)>(vals, lane);
          if (my_slot >= 0) s_acc[j][my_slot] = tot;
        } else {
#pragma unroll
          for (int base = 0; base < NACC; base += 16) {
            float vals[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
              const int k = base + c;
              vals[c] = k < NS ? S[k < NS ? k : 0] : (k < NACC ? gf[(k - NS) < FP && k >= NS ? (k - NS) : 0] : 0.0f);
            }
            const float tot = gs_wave_reduce16_transposed(vals, lane);
            const int k = base + (lane >> 2);
            if ((lane & 3) == 0 && k < NACC) s_acc[j][k] = tot;
          }
        }
      }
    }
    __syncthreads();

    // ---- per-splat epilogue: lane j turns splat j's totals into its gradient row
    {
      float row[ROW];
#pragma unroll
      for (int c = 0; c < ROW; ++c) row[c] = 0.0f;
      if (lane < cnt) {
        float t[NACC];
#pragma unroll
        for (int c = 0; c < NACC; ++c) t[c] = s_acc[lane][c];
        if (FULL) {
#pragma unroll
          for (int c = 0; c < 7; ++c) row[c] = t[c];
          if (a.aa) gs_mean_grad_from_splat_frame(row[0], row[1], ax, ay);
          if (a.heur) { row[7 + FP] = t[7]; row[8 + FP] = t[8]; }
        } else {
          // t = wave totals of (G, G tx, G ty, G tx^2, G tx ty, G ty^2), tx = d.axis/sx, ty = d.perp(axis)/sy.
          // With d = (sx tx axis + sy ty perp(axis)) / |axis|^2 the position-weighted sums follow:
          //   sum G tx d = (sx Mxx axis + sy Mxy perp) / n2 ,  sum G ty d = (sx Mxy axis + sy Myy perp) / n2
          // and dp/dmean, dp/daxis, dp/dsigma (taichi_lib/generic.py:321-336) become
          // the totals carry alpha_p (G = alpha_p pdf dL/dalpha) and powers of K_EXP (scaled tx, ty): undo both here
          t[1] *= IK; t[2] *= IK;
          t[3] *= IK2; t[4] *= IK2; t[5] *= IK2;
          const float sx = gs_rcp_fast(isx), sy = gs_rcp_fast(isy);
          const float in2 = gs_rcp_fast(ax * ax + ay * ay);
          const float txdx = (sx * ax * t[3] - sy * ay * t[4]) * in2, txdy = (sx * ay * t[3] + sy * ax * t[4]) * in2;
          const float tydx = (sx * ax * t[4] - sy * ay * t[5]) * in2, tydy = (sx * ay * t[4] + sy * ax * t[5]) * in2;
          row[0] = t[1] * isx * ax - t[2] * isy * ay;
          row[1] = t[1] * isx * ay + t[2] * isy * ax;
          row[2] = -(isx * txdx + isy * tydy);
          row[3] = isy * tydx - isx * txdy;
          row[4] = t[3] * isx;
          row[5] = t[5] * isy;
          // G carries the opacity; a listed splat at or below the threshold (a caller's own tile lists may hold one:
          // opacity zeroed after map_to_tiles) blended nothing, and 0 * rcp(0) must not become NaN
          row[6] = al > a.thr ? t[0] * gs_rcp_fast(al) : 0.0f;
          if (HEUR) { row[7 + FP] = t[6] * al * al; row[8 + FP] = t[7] * IK2; }
        }
#pragma unroll
        for (int c = 0; c < FP; ++c) row[7 + c] = t[NS + c];
        // the Gaussian's row index (still in this lane's register from the staging) rides in the row's last, unused
        // word to the flush below: no index array in LDS
        static_assert(9 + FP < ROW, "the gradient row needs a spare word");
        row[ROW - 1] = __int_as_float(idx);
      }
      __syncthreads();  // `out` aliases the totals just read
#pragma unroll
      for (int c = 0; c < ROW; ++c) s_out[lane][c] = row[c];
    }
    __syncthreads();
    // ---- flush: 64/ROW splats x ROW contiguous floats per wave atomic instruction
    for (int e = lane; e < cnt * ROW; e += 64) {
      const int jj = e / ROW, comp = e - jj * ROW;
      const float val = s_out[jj][comp];
      // heuristics live at [7+F, 9+F) of the caller's row; the kernel's padded slot is 7+FP
      int dst = comp;
      if (comp >= 9 + FP) continue;  // padding, and the index word
      if (comp >= 7 + FP) dst = comp - FP + a.F;
      else if (comp >= 7 + a.F) continue;
      if (val != 0.0f)
        atomicAdd(a.grad_rows + int64_t(__float_as_int(s_out[jj][ROW - 1])) * a.row_floats + dst, val);
    }
    __syncthreads();
  }
}

// Block -> work: gs_raster_region (raster_walk.h; the mapper's fullest tiles get one workgroup per 8x8 quadrant).
template <int NB, int FP, int MODE>
__global__ __launch_bounds__(64) void raster_bwd_kernel(const BwdArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[BwdShape<FP, MODE>::ARENA_F];
  // the 64-byte block of zeros that every splat's sums start from (raster_bwd_body)
  __shared__ __attribute__((aligned(16))) float s_zeros[16];
  if (threadIdx.x < 16) s_zeros[threadIdx.x] = 0.0f;  // read after the first staging barrier
  gs_raster_region<NB>(a, [&](auto nb, int tile, int x0, int y0, int yout0) {
    raster_bwd_body<decltype(nb)::value, FP, MODE>(a, tile, x0, y0, yout0, smem, s_zeros);
  });
}

template <int NB, int MODE>
int launch_fp(const BwdArgs& a, hipStream_t s) {
  const int grid = gs_raster_grid(a);
  if (a.F <= 3) hipLaunchKernelGGL((raster_bwd_kernel<NB, 3, MODE>), dim3(grid), dim3(64), 0, s, a);
  else if (a.F <= 5) hipLaunchKernelGGL((raster_bwd_kernel<NB, 5, MODE>), dim3(grid), dim3(64), 0, s, a);
  else if (a.F <= 8) hipLaunchKernelGGL((raster_bwd_kernel<NB, 8, MODE>), dim3(grid), dim3(64), 0, s, a);
  else hipLaunchKernelGGL((raster_bwd_kernel<NB, 32, MODE>), dim3(grid), dim3(64), 0, s, a);
  GS_CHECK_LAUNCH("gs_raster_bwd");
  return GS_OK;
}

__global__ void unpack_kernel(int64_t v, int F, int row_floats, const float* rows, float* gp, float* gf, float* heur) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int per = 9 + F;
  if (i >= v * per) return;
  const int64_t r = i / per;
  const int c = int(i - r * per);
  const float val = rows[r * row_floats + c];
  if (c < 7) { if (gp) gp[r * 7 + c] = val; }
  else if (c < 7 + F) { if (gf) gf[r * F + (c - 7)] = val; }
  else if (heur) heur[r * 2 + (c - 7 - F)] = val;
}

}  // namespace

extern "C" int32_t gs_grad_row_floats(int32_t num_features) { return int32_t(gs_align_up(9 + num_features, 16)); }

extern "C" int gs_raster_bwd(int64_t v, int32_t num_features, const float* points, const float* features,
                             const int32_t* tile_ranges, const int32_t* overlap_to_point, int64_t k, int32_t width,
                             int32_t height, const GsRasterConfig* cfg, const int32_t* tile_order,
                             const int32_t* heavy_tiles, const float* image, const float* grad_image,
                             const float* alpha, const float* grad_weight, float* grad_rows, const GsRowShard* shard,
                             void* stream) {
  if (int rc = gs_check_cfg(cfg)) return rc;
  GS_REQUIRE(!grad_weight || alpha, GS_ERR_INVALID_ARGUMENT,
             "gs_raster_bwd: grad_weight without the forward's alpha image");
  if (int rc = gs_check_raster_call("gs_raster_bwd", width, height, num_features, GS_MAX_FEATURES)) return rc;
  GS_REQUIRE(image && grad_image && tile_ranges, GS_ERR_INVALID_ARGUMENT, "gs_raster_bwd: NULL image or ranges");
  GS_REQUIRE(cfg->use_alpha_blending, GS_ERR_UNSUPPORTED,
             "gs_raster_bwd: no gradient is defined without alpha blending (reference tests/test_rasterizer.py:92-101)");
  if (k == 0 || v == 0) return GS_OK;
  GS_REQUIRE(points && features && overlap_to_point && grad_rows, GS_ERR_INVALID_ARGUMENT,
             "gs_raster_bwd: NULL input");
  BwdArgs a;
  a.points = points; a.features = features; a.ranges = reinterpret_cast<const int2*>(tile_ranges);
  a.o2p = overlap_to_point; a.image = image; a.grad_image = grad_image; a.grad_rows = grad_rows;
  a.W = width; a.H = height; a.F = num_features;
  a.row_floats = gs_grad_row_floats(num_features);
  int nb = 0;
  if (int rc = gs_raster_geometry(a, cfg, width, height, tile_order, heavy_tiles, shard, 1, nb)) return rc;
  if (a.num_tiles == 0) return GS_OK;
  a.cmax = cfg->clamp_max_alpha; a.thr = cfg->alpha_threshold; a.sat = cfg->saturate_threshold;
  a.inv_thr = 1.0f / cfg->alpha_threshold;
  a.aa = cfg->antialias; a.heur = cfg->compute_point_heuristic;
  a.alpha = alpha; a.grad_weight = grad_weight;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int mode = a.aa ? 2 : a.heur ? 1 : 0;
  if (nb == 1) return mode == 2 ? launch_fp<1, 2>(a, s) : mode == 1 ? launch_fp<1, 1>(a, s) : launch_fp<1, 0>(a, s);
  if (nb == 2) return mode == 2 ? launch_fp<2, 2>(a, s) : mode == 1 ? launch_fp<2, 1>(a, s) : launch_fp<2, 0>(a, s);
  return mode == 2 ? launch_fp<4, 2>(a, s) : mode == 1 ? launch_fp<4, 1>(a, s) : launch_fp<4, 0>(a, s);
}

extern "C" int gs_raster_bwd_unpack(int64_t v, int32_t num_features, const float* grad_rows, float* grad_points,
                                    float* grad_features, float* point_heuristic, void* stream) {
  if (v == 0) return GS_OK;
  GS_REQUIRE(grad_rows, GS_ERR_INVALID_ARGUMENT, "gs_raster_bwd_unpack: grad_rows is NULL");
  const int64_t total = v * (9 + num_features);
  hipLaunchKernelGGL(unpack_kernel, dim3(unsigned(gs_div_up(total, 256))), dim3(256), 0,
                     static_cast<hipStream_t>(stream), v, num_features, gs_grad_row_floats(num_features), grad_rows,
                     grad_points, grad_features, point_heuristic);
  GS_CHECK_LAUNCH("gs_raster_bwd_unpack");
  return GS_OK;
}
