// envmap.hip -- a learnable cubemap environment behind a render, forward and backward (gfx950), float and double.
//
// Per pixel (column x, row y) of a pinhole camera with projection (fx, fy, cx, cy) and world -> camera matrix T:
//   d_cam = ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1),   d = Rcw^T d_cam,  Rcw = T[:3, :3] taken as a rotation
//   a = the axis of the largest |d_i| (ties to the lower index),  face = 2 a + (d_a < 0)
//   (p, q) = the two other components in ascending axis order, divided by |d_a|
//   u = clamp((p + 1) / 2 * R - 0.5, 0, R - 1) (column),  v = clamp((q + 1) / 2 * R - 0.5, 0, R - 1) (row)
//   sky = bilinear interpolation of env[face] at (v, u), taps clamped inside the face
//   out = image + (1 - weight) * sky
// No sign flips between faces and no filtering across face seams.  Interpolation is a + (b - a) * f along u, then v:
// where the four taps agree the result is the tap, so a constant map returns the constant bit for bit.
//
// Forward and the weight's gradient: one lane per pixel.
//
// The map's gradient is a gather, one sum per texel, no atomics: a cube face is a 90-degree pinhole image, so a texel's
// bilinear support (+-1 texel about its centre, clipped to the face) is a convex quadrilateral of the face plane and
// projects to a convex quadrilateral of the image as long as its four corners lie in front of the camera.  A texel
// first tests its centre against the camera's cone (the largest angle an image corner makes with the optical axis, plus
// the angle its support can subtend): outside, it writes zeros.  Inside, it projects the four corners, takes their
// bounding box, padded by a quarter of a pixel and clipped to the image -- the whole image when a corner is not clearly
// in front of the camera -- and runs env_pixel, the forward's own function, on every pixel of the box: a pixel adds
// its term only if env_pixel names this texel as one of its taps.  The box only has to be conservative; every index
// that addresses a tensor is clamped by env_pixel or comes from the clipped box.
//   lane kernel  (fine maps, a few pixels per texel): one lane per texel walks its box.
//   group kernel (coarse maps): 1 or 4 waves per texel, the lanes stride over the box; where the texels in view are
//                too few to fill the chip, a box is cut into `slices` interleaved parts whose sums a second launch
//                adds in slice order.
// Every sum has one program order given the shapes: the outputs repeat bit for bit.
// The host picks the kernel from R and the image size alone (the focal length lives on the device and is not read
// back): it takes a texel to cover max(W, H) / R pixels a side, which is exact for a 90-degree field of view.
#include <cmath>

#include "gs_common.h"

namespace {

constexpr int ENV_MAX_C = 4;
constexpr int ENV_MAX_R = 16384;
constexpr int ENV_THREADS = 256;
constexpr int ENV_MAX_SLICES = 64;
constexpr int64_t ENV_MIN_WAVES = 8192;    // waves at work that fill the chip: eight on every SIMD
constexpr int64_t ENV_VIEW_SHARE = 6;      // the host takes one texel in six to lie in the camera's cone (one face)
constexpr double ENV_LANE_BELOW = 256.0;   // estimated pixels in a texel's box: below, one lane per texel
constexpr double ENV_WAVE_BELOW = 1024.0;  // below, one wave per texel; from here on, four

template <typename T>
struct EnvCam {
  T fx, fy, cx, cy;
  T m[9];  // Rcw, row-major
};

template <typename T>
__device__ __forceinline__ EnvCam<T> env_camera(const T* projection, const T* T_camera_world) {
  EnvCam<T> c;
  c.fx = projection[0]; c.fy = projection[1]; c.cx = projection[2]; c.cy = projection[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) c.m[3 * r + k] = T_camera_world[4 * r + k];
  return c;
}

template <typename T>
struct EnvTap {
  int face, i0, j0, i1, j1;  // all inside [0, 6) and [0, R) whatever the camera holds
  T fu, fv;
};

// the one place a pixel is turned into a face and its taps: forward and backward share it
template <typename T>
__device__ __forceinline__ EnvTap<T> env_pixel(const EnvCam<T>& c, int R, int x, int y) {
  const T dx = (T(x) + T(0.5) - c.cx) / c.fx, dy = (T(y) + T(0.5) - c.cy) / c.fy;
  const T d0 = c.m[0] * dx + c.m[3] * dy + c.m[6];
  const T d1 = c.m[1] * dx + c.m[4] * dy + c.m[7];
  const T d2 = c.m[2] * dx + c.m[5] * dy + c.m[8];
  const T a0 = fabs(d0), a1 = fabs(d1), a2 = fabs(d2);
  int axis = 0;
  T da = d0, ad = a0, p = d1, q = d2;
  if (a1 > ad) { axis = 1; da = d1; ad = a1; p = d0; q = d2; }
  if (a2 > ad) { axis = 2; da = d2; ad = a2; p = d0; q = d1; }
  EnvTap<T> t;
  t.face = 2 * axis + (da < T(0) ? 1 : 0);
  const T top = T(R - 1);
  // fmin / fmax drop a NaN: the taps stay inside the face whatever the camera holds
  const T u = fmax(fmin((p / ad + T(1)) * T(0.5) * T(R) - T(0.5), top), T(0));
  const T v = fmax(fmin((q / ad + T(1)) * T(0.5) * T(R) - T(0.5), top), T(0));
  t.i0 = int(u);
  t.j0 = int(v);
  t.i1 = t.i0 + 1 < R ? t.i0 + 1 : R - 1;
  t.j1 = t.j0 + 1 < R ? t.j0 + 1 : R - 1;
  t.fu = u - T(t.i0);
  t.fv = v - T(t.j0);
  return t;
}

template <typename T>
struct EnvArgs {
  int height, width, channels, R;
  const T* env;         // (6, R, R, C)
  const T* image;       // NULL: the sky alone
  int64_t isr, isp;
  const T* weight;      // NULL with image
  int64_t wsr, wsp;
  const T* projection;  // 4, device
  const T* pose;        // 16, device
  T* out;               // forward: (H, W, C)
  const T* grad_out;    // backward: (H, W, C)
  T* d_weight;          // (H, W), or NULL
  T* d_env;             // (6, R, R, C), or NULL
  T* partials;          // (texel, slice, C) when slices > 1
  int slices;
};

template <typename T, int C>
__device__ __forceinline__ void env_sky(const EnvArgs<T>& a, const EnvTap<T>& t, T (&sky)[C]) {
  const int64_t face = int64_t(t.face) * a.R;
  const T* r0 = a.env + (face + t.j0) * a.R * C;
  const T* r1 = a.env + (face + t.j1) * a.R * C;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const T v00 = r0[int64_t(t.i0) * C + c], v01 = r0[int64_t(t.i1) * C + c];
    const T v10 = r1[int64_t(t.i0) * C + c], v11 = r1[int64_t(t.i1) * C + c];
    const T top = v00 + (v01 - v00) * t.fu;
    const T bot = v10 + (v11 - v10) * t.fu;
    sky[c] = top + (bot - top) * t.fv;
  }
}

// BWD = false: out = image + (1 - weight) sky.  BWD = true: d_weight = -sum_c grad_out_c sky_c.
template <typename T, int C, bool BWD>
__global__ __launch_bounds__(ENV_THREADS) void envmap_pixel_kernel(EnvArgs<T> a) {
  const int64_t pix = int64_t(blockIdx.x) * ENV_THREADS + threadIdx.x;
  if (pix >= int64_t(a.height) * a.width) return;
  const int y = int(pix / a.width), x = int(pix - int64_t(y) * a.width);
  const EnvCam<T> cam = env_camera(a.projection, a.pose);
  const EnvTap<T> t = env_pixel(cam, a.R, x, y);
  T sky[C];
  env_sky<T, C>(a, t, sky);
  if (BWD) {
    const T* g = a.grad_out + pix * C;
    T sum = T(0);
#pragma unroll
    for (int c = 0; c < C; ++c) sum += g[c] * sky[c];
    a.d_weight[pix] = -sum;
  } else {
    T* o = a.out + pix * C;
    if (a.image) {
      const T* ip = a.image + int64_t(y) * a.isr + int64_t(x) * a.isp;
      const T k = T(1) - a.weight[int64_t(y) * a.wsr + int64_t(x) * a.wsp];
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = ip[c] + k * sky[c];
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = sky[c];
    }
  }
}

// ------------------------------------------------------------------------------------------ the map's gradient
struct EnvBox {
  int x0, y0, x1, y1;  // inclusive, inside the image; x0 > x1: empty
};

// cos of the widest angle between the optical axis and a texel centre whose support a pixel can fall in:
// cos(theta + delta) from tan(theta) = the farthest image corner and delta = the most the support's half diagonal on
// the face plane, s = 2 sqrt(2) / R, can subtend (a segment of length s on a plane at distance >= 1 subtends at most
// 2 atan(s / 2), whose tangent is s / (1 - s^2 / 4)), both tangents taken 5 % + 0.01 larger.  R <= 2: every texel passes.
template <typename T>
__device__ __forceinline__ T env_cone_cos(const EnvCam<T>& c, int R, int width, int height) {
  if (R <= 2) return T(-1);
  const T xl = (T(0) - c.cx) / c.fx, xr = (T(width) - c.cx) / c.fx;
  const T yt = (T(0) - c.cy) / c.fy, yb = (T(height) - c.cy) / c.fy;
  const T tx = fmax(fabs(xl), fabs(xr)), ty = fmax(fabs(yt), fabs(yb));
  const T t = sqrt(tx * tx + ty * ty) * T(1.05) + T(0.01);
  const T h = T(1.4142135623730951) / T(R);  // s / 2 <= 0.4714
  const T s = T(2) * h / (T(1) - h * h) * T(1.05) + T(0.01);
  const T cosine = (T(1) - t * s) / sqrt((T(1) + t * t) * (T(1) + s * s));
  return cosine == cosine ? cosine : T(-1);  // a camera of NaNs rejects nothing
}

// face coordinates -> camera coordinates of the direction with component `axis` = sign, the others p, q
template <typename T>
__device__ __forceinline__ void env_to_camera(const EnvCam<T>& c, int axis, T sign, T p, T q, T (&X)[3]) {
  const T D0 = axis == 0 ? sign : p;
  const T D1 = axis == 0 ? p : (axis == 1 ? sign : q);
  const T D2 = axis == 2 ? sign : q;
#pragma unroll
  for (int k = 0; k < 3; ++k) X[k] = c.m[3 * k] * D0 + c.m[3 * k + 1] * D1 + c.m[3 * k + 2] * D2;
}

template <typename T>
__device__ __forceinline__ int env_clip(T v, int top) {  // v rounded already; NaN -> 0
  return int(fmax(fmin(v, T(top)), T(0)));
}

// the pixels that can hold texel (face, j, i) as a tap: conservative, inside the image
template <typename T>
__device__ __forceinline__ EnvBox env_box(const EnvCam<T>& c, T cone_cos, int R, int width, int height, int face, int j,
                                          int i) {
  EnvBox b = {1, 1, 0, 0};
  const int axis = face >> 1;
  const T sign = (face & 1) ? T(-1) : T(1);
  const T step = T(2) / T(R);
  const T pc = (T(i) + T(0.5)) * step - T(1), qc = (T(j) + T(0.5)) * step - T(1);
  T X[3];
  env_to_camera(c, axis, sign, pc, qc, X);
  if (X[2] < cone_cos * sqrt(T(1) + pc * pc + qc * qc)) return b;
  const T pe[2] = {fmax(pc - step, T(-1)), fmin(pc + step, T(1))};
  const T qe[2] = {fmax(qc - step, T(-1)), fmin(qc + step, T(1))};
  T xlo = T(1e30), xhi = T(-1e30), ylo = T(1e30), yhi = T(-1e30);
  bool front = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    env_to_camera(c, axis, sign, pe[k & 1], qe[k >> 1], X);
    front = front && X[2] > T(0.02);  // |direction| <= sqrt(3): more than 0.6 degrees in front of the camera's plane
    const T px = c.fx * (X[0] / X[2]) + c.cx, py = c.fy * (X[1] / X[2]) + c.cy;
    xlo = fmin(xlo, px); xhi = fmax(xhi, px);
    ylo = fmin(ylo, py); yhi = fmax(yhi, py);
  }
  if (!front) {
    b.x0 = 0; b.y0 = 0; b.x1 = width - 1; b.y1 = height - 1;
    return b;
  }
  // pixel centres x + 0.5 inside [xlo - 1/4, xhi + 1/4]
  b.x0 = env_clip(ceil(xlo - T(0.75)), width);
  b.x1 = env_clip(floor(xhi - T(0.25)), width - 1);
  b.y0 = env_clip(ceil(ylo - T(0.75)), height);
  b.y1 = env_clip(floor(yhi - T(0.25)), height - 1);
  if (b.y0 > b.y1) { b.x0 = 1; b.x1 = 0; }
  return b;
}

// what pixel (x, y) adds to texel (face, j, i): acc += (1 - weight) * tap weight * grad_out
template <typename T, int C>
__device__ __forceinline__ void env_gather(const EnvArgs<T>& a, const EnvCam<T>& cam, int face, int j, int i, int x,
                                           int y, T (&acc)[C]) {
  const EnvTap<T> t = env_pixel(cam, a.R, x, y);
  if (t.face != face) return;
  // the upper tap is a texel of its own only where it exists: i0 + 1 == R never equals i
  const T wu = (t.i0 == i ? T(1) - t.fu : T(0)) + (t.i0 + 1 == i ? t.fu : T(0));
  const T wv = (t.j0 == j ? T(1) - t.fv : T(0)) + (t.j0 + 1 == j ? t.fv : T(0));
  const bool member = (t.i0 == i || t.i0 + 1 == i) && (t.j0 == j || t.j0 + 1 == j);
  if (!member) return;
  T k = wu * wv;
  if (a.weight) k *= T(1) - a.weight[int64_t(y) * a.wsr + int64_t(x) * a.wsp];
  const T* g = a.grad_out + (int64_t(y) * a.width + x) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] += k * g[c];
}

template <typename T, int C>
__global__ __launch_bounds__(ENV_THREADS) void envmap_texel_lane_kernel(EnvArgs<T> a) {
  const int64_t texels = int64_t(6) * a.R * a.R;
  const int64_t t = int64_t(blockIdx.x) * ENV_THREADS + threadIdx.x;
  if (t >= texels) return;
  const int i = int(t % a.R), j = int((t / a.R) % a.R), face = int(t / (int64_t(a.R) * a.R));
  const EnvCam<T> cam = env_camera(a.projection, a.pose);
  const EnvBox b = env_box(cam, env_cone_cos(cam, a.R, a.width, a.height), a.R, a.width, a.height, face, j, i);
  T acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = T(0);
  if (b.x0 <= b.x1)
    for (int y = b.y0; y <= b.y1; ++y)
      for (int x = b.x0; x <= b.x1; ++x) env_gather<T, C>(a, cam, face, j, i, x, y, acc);
#pragma unroll
  for (int c = 0; c < C; ++c) a.d_env[t * C + c] = acc[c];
}

// WAVES waves per texel, ENV_THREADS / 64 / WAVES texels per workgroup, a.slices workgroups per texel group: slice s
// takes the box's pixels s * LANES + lane, then every slices * LANES-th
template <typename T, int C, int WAVES>
__global__ __launch_bounds__(ENV_THREADS) void envmap_texel_group_kernel(EnvArgs<T> a) {
  constexpr int LANES = GS_WAVE * WAVES, PER_BLOCK = ENV_THREADS / LANES;
  __shared__ T s_part[ENV_THREADS / GS_WAVE][ENV_MAX_C];
  const int64_t texels = int64_t(6) * a.R * a.R;
  const int slice = int(blockIdx.x % unsigned(a.slices));
  const int64_t group = int64_t(blockIdx.x / unsigned(a.slices));
  const int member = threadIdx.x % LANES, wave = threadIdx.x / GS_WAVE;
  const int64_t t = group * PER_BLOCK + threadIdx.x / LANES;
  const bool live = t < texels;  // the same for every lane of a wave
  T acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = T(0);
  if (live) {
    const int i = int(t % a.R), j = int((t / a.R) % a.R), face = int(t / (int64_t(a.R) * a.R));
    const EnvCam<T> cam = env_camera(a.projection, a.pose);
    const EnvBox b = env_box(cam, env_cone_cos(cam, a.R, a.width, a.height), a.R, a.width, a.height, face, j, i);
    if (b.x0 <= b.x1) {
      const unsigned bw = unsigned(b.x1 - b.x0 + 1);
      const unsigned n = bw * unsigned(b.y1 - b.y0 + 1);  // height * width < 2^31: 32-bit divisions
      const unsigned stride = unsigned(a.slices) * LANES;  // <= 2^14
      for (unsigned e = unsigned(slice) * LANES + member; e < n; e += stride) {
        const unsigned row = e / bw, col = e - row * bw;
        env_gather<T, C>(a, cam, face, j, i, b.x0 + int(col), b.y0 + int(row), acc);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[c] += __shfl_xor(acc[c], off);
  if (WAVES > 1) {
    if ((threadIdx.x & (GS_WAVE - 1)) == 0)
#pragma unroll
      for (int c = 0; c < C; ++c) s_part[wave][c] = acc[c];
    __syncthreads();
    if (member == 0)
#pragma unroll
      for (int c = 0; c < C; ++c) {
        T sum = s_part[wave][c];
        for (int w = 1; w < WAVES; ++w) sum += s_part[wave + w][c];
        acc[c] = sum;
      }
  }
  if (!live || member != 0) return;
  T* dst = a.slices > 1 ? a.partials + (t * a.slices + slice) * C : a.d_env + t * C;
#pragma unroll
  for (int c = 0; c < C; ++c) dst[c] = acc[c];
}

// d_env[e] = the slices' sums of element e, in slice order
template <typename T>
__global__ __launch_bounds__(ENV_THREADS) void envmap_finish_kernel(EnvArgs<T> a) {
  const int64_t e = int64_t(blockIdx.x) * ENV_THREADS + threadIdx.x;
  if (e >= int64_t(6) * a.R * a.R * a.channels) return;
  const int64_t t = e / a.channels;
  const int c = int(e - t * a.channels);
  const T* p = a.partials + t * a.slices * a.channels + c;
  T sum = T(0);
  for (int s = 0; s < a.slices; ++s) sum += p[int64_t(s) * a.channels];
  a.d_env[e] = sum;
}

// ------------------------------------------------------------------------------------------------------------- host
struct EnvPlan {
  int waves;   // 0: the lane kernel
  int slices;
  int64_t blocks;
};

int env_sizes(const char* who, int64_t height, int64_t width, int64_t channels, int64_t R) {
  GS_REQUIRE(height >= 1 && width >= 1, GS_ERR_INVALID_ARGUMENT, "%s: image %lld x %lld is empty", who,
             (long long)height, (long long)width);
  GS_REQUIRE(R >= 1, GS_ERR_INVALID_ARGUMENT, "%s: map edge %lld", who, (long long)R);
  GS_REQUIRE(channels >= 1 && channels <= ENV_MAX_C, GS_ERR_UNSUPPORTED, "%s: %lld channels not in [1,%d]", who,
             (long long)channels, ENV_MAX_C);
  GS_REQUIRE(R <= ENV_MAX_R, GS_ERR_UNSUPPORTED, "%s: map edge %lld above %d", who, (long long)R, ENV_MAX_R);
  GS_REQUIRE(height < (int64_t(1) << 31) && width < (int64_t(1) << 31) && height * width < (int64_t(1) << 31),
             GS_ERR_UNSUPPORTED, "%s: image %lld x %lld above 2^31 pixels", who, (long long)height, (long long)width);
  return GS_OK;
}

// which kernel adds the map's gradient: from the pixels a texel's box would hold under a 90-degree field of view
EnvPlan env_plan(int64_t height, int64_t width, int64_t R) {
  const int64_t texels = 6 * R * R;
  const double side = 2.0 * double(width > height ? width : height) / double(R) + 1.0, box = side * side;
  EnvPlan p;
  if (box < ENV_LANE_BELOW) {
    p.waves = 0; p.slices = 1; p.blocks = gs_div_up(texels, ENV_THREADS);
    return p;
  }
  p.waves = box < ENV_WAVE_BELOW ? 1 : 4;
  const int lanes = GS_WAVE * p.waves;
  const int64_t groups = gs_div_up(texels, ENV_THREADS / lanes);
  int64_t slices = gs_div_up(ENV_MIN_WAVES * ENV_VIEW_SHARE, texels * p.waves);
  const int64_t useful = int64_t(box / (4.0 * lanes));  // a slice keeps four pixels per lane
  slices = slices < useful ? slices : useful;
  slices = slices > ENV_MAX_SLICES ? ENV_MAX_SLICES : (slices < 1 ? 1 : slices);
  p.slices = int(slices);
  p.blocks = groups * slices;
  return p;
}

int64_t env_scratch_bytes(const EnvPlan& p, int64_t channels, int64_t R, size_t elem) {
  return p.slices > 1 ? 6 * R * R * p.slices * channels * int64_t(elem) : 0;
}

template <typename T>
int env_common(const char* who, int64_t height, int64_t width, int64_t channels, const T* env, int64_t R,
               const T* weight, int64_t wsr, int64_t wsp, const T* projection, const T* pose, EnvArgs<T>* a) {
  GS_TRY(env_sizes(who, height, width, channels, R));
  GS_REQUIRE(projection != nullptr && pose != nullptr, GS_ERR_INVALID_ARGUMENT,
             "%s: NULL buffer (projection / T_camera_world)", who);
  if (weight)
    GS_REQUIRE(wsp >= 1 && wsr >= width * wsp, GS_ERR_INVALID_ARGUMENT,
               "%s: bad strides of weight (row %lld, pixel %lld elements for %lld x %lld)", who, (long long)wsr,
               (long long)wsp, (long long)height, (long long)width);
  a->height = int(height); a->width = int(width); a->channels = int(channels); a->R = int(R);
  a->env = env; a->image = nullptr; a->isr = 0; a->isp = 0;
  a->weight = weight; a->wsr = wsr; a->wsp = wsp;
  a->projection = projection; a->pose = pose;
  a->out = nullptr; a->grad_out = nullptr; a->d_weight = nullptr; a->d_env = nullptr; a->partials = nullptr;
  a->slices = 1;
  return GS_OK;
}

template <typename T, bool BWD>
void env_launch_pixels(const EnvArgs<T>& a, hipStream_t st) {
  const unsigned blocks = unsigned(gs_div_up(int64_t(a.height) * a.width, ENV_THREADS));
  switch (a.channels) {
    case 1: hipLaunchKernelGGL((envmap_pixel_kernel<T, 1, BWD>), dim3(blocks), dim3(ENV_THREADS), 0, st, a); break;
    case 2: hipLaunchKernelGGL((envmap_pixel_kernel<T, 2, BWD>), dim3(blocks), dim3(ENV_THREADS), 0, st, a); break;
    case 3: hipLaunchKernelGGL((envmap_pixel_kernel<T, 3, BWD>), dim3(blocks), dim3(ENV_THREADS), 0, st, a); break;
    default: hipLaunchKernelGGL((envmap_pixel_kernel<T, 4, BWD>), dim3(blocks), dim3(ENV_THREADS), 0, st, a); break;
  }
}

template <typename T, int C>
void env_launch_texels(const EnvArgs<T>& a, const EnvPlan& p, hipStream_t st) {
  const dim3 grid(unsigned(p.blocks)), block(ENV_THREADS);
  if (p.waves == 0) hipLaunchKernelGGL((envmap_texel_lane_kernel<T, C>), grid, block, 0, st, a);
  else if (p.waves == 1) hipLaunchKernelGGL((envmap_texel_group_kernel<T, C, 1>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((envmap_texel_group_kernel<T, C, 4>), grid, block, 0, st, a);
}

template <typename T>
int env_fwd(const char* who, int64_t height, int64_t width, int64_t channels, const T* env, int64_t R, const T* image,
            int64_t isr, int64_t isp, const T* weight, int64_t wsr, int64_t wsp, const T* projection, const T* pose,
            T* out, void* stream) {
  EnvArgs<T> a;
  GS_TRY(env_common(who, height, width, channels, env, R, weight, wsr, wsp, projection, pose, &a));
  GS_REQUIRE(env != nullptr && out != nullptr, GS_ERR_INVALID_ARGUMENT, "%s: NULL buffer (env / out)", who);
  GS_REQUIRE((image == nullptr) == (weight == nullptr), GS_ERR_INVALID_ARGUMENT,
             "%s: image and weight go together (both, or both NULL for the sky alone)", who);
  if (image)
    GS_REQUIRE(isp >= channels && isr >= width * isp, GS_ERR_INVALID_ARGUMENT,
               "%s: bad strides of image (row %lld, pixel %lld elements for %lld x %lld x %lld)", who, (long long)isr,
               (long long)isp, (long long)height, (long long)width, (long long)channels);
  a.image = image; a.isr = isr; a.isp = isp; a.out = out;
  env_launch_pixels<T, false>(a, static_cast<hipStream_t>(stream));
  GS_CHECK_LAUNCH(who);
  return GS_OK;
}

template <typename T>
int env_bwd(const char* who, int64_t height, int64_t width, int64_t channels, const T* env, int64_t R, const T* weight,
            int64_t wsr, int64_t wsp, const T* projection, const T* pose, const T* grad_out, T* d_weight, T* d_env,
            void* scratch, int64_t scratch_bytes, void* stream) {
  EnvArgs<T> a;
  GS_TRY(env_common(who, height, width, channels, env, R, weight, wsr, wsp, projection, pose, &a));
  GS_REQUIRE(grad_out != nullptr, GS_ERR_INVALID_ARGUMENT, "%s: NULL buffer (grad_out)", who);
  GS_REQUIRE(d_weight || d_env, GS_ERR_INVALID_ARGUMENT, "%s: NULL buffer (no gradient asked for)", who);
  GS_REQUIRE(!d_weight || (weight && env), GS_ERR_INVALID_ARGUMENT, "%s: d_weight without a weight or without env",
             who);
  const EnvPlan plan = env_plan(height, width, R);
  if (d_env) {
    GS_REQUIRE(plan.blocks < (int64_t(1) << 31), GS_ERR_UNSUPPORTED, "%s: %lld workgroups above the launch limit 2^31",
               who, (long long)plan.blocks);
    const int64_t need = env_scratch_bytes(plan, channels, R, sizeof(T));
    if (need > 0) {
      GS_TRY(gs_check_scratch(who, scratch, scratch_bytes, need));
      a.partials = static_cast<T*>(scratch);
    }
    a.slices = plan.slices;
  }
  a.grad_out = grad_out; a.d_weight = d_weight; a.d_env = d_env;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (d_weight) {
    env_launch_pixels<T, true>(a, st);
    GS_CHECK_LAUNCH(who);
  }
  if (d_env) {
    switch (a.channels) {
      case 1: env_launch_texels<T, 1>(a, plan, st); break;
      case 2: env_launch_texels<T, 2>(a, plan, st); break;
      case 3: env_launch_texels<T, 3>(a, plan, st); break;
      default: env_launch_texels<T, 4>(a, plan, st); break;
    }
    GS_CHECK_LAUNCH(who);
    if (plan.slices > 1) {
      const unsigned blocks = unsigned(gs_div_up(6 * R * R * channels, ENV_THREADS));
      hipLaunchKernelGGL(envmap_finish_kernel<T>, dim3(blocks), dim3(ENV_THREADS), 0, st, a);
      GS_CHECK_LAUNCH(who);
    }
  }
  return GS_OK;
}

}  // namespace

extern "C" int64_t gs_envmap_scratch_bytes(int64_t height, int64_t width, int64_t channels, int64_t map_edge,
                                            int32_t f64) {
  GS_TRY(env_sizes("gs_envmap_scratch_bytes", height, width, channels, map_edge));
  return env_scratch_bytes(env_plan(height, width, map_edge), channels, map_edge, f64 ? sizeof(double) : sizeof(float));
}

extern "C" int gs_envmap_fwd(int64_t height, int64_t width, int64_t channels, const float* env, int64_t map_edge,
                             const float* image, int64_t image_row_stride, int64_t image_pixel_stride,
                             const float* weight, int64_t weight_row_stride, int64_t weight_pixel_stride,
                             const float* projection, const float* T_camera_world, float* out, void* stream) {
  return env_fwd<float>("gs_envmap_fwd", height, width, channels, env, map_edge, image, image_row_stride,
                        image_pixel_stride, weight, weight_row_stride, weight_pixel_stride, projection, T_camera_world,
                        out, stream);
}

extern "C" int gs_envmap_fwd_f64(int64_t height, int64_t width, int64_t channels, const double* env, int64_t map_edge,
                                 const double* image, int64_t image_row_stride, int64_t image_pixel_stride,
                                 const double* weight, int64_t weight_row_stride, int64_t weight_pixel_stride,
                                 const double* projection, const double* T_camera_world, double* out, void* stream) {
  return env_fwd<double>("gs_envmap_fwd_f64", height, width, channels, env, map_edge, image, image_row_stride,
                         image_pixel_stride, weight, weight_row_stride, weight_pixel_stride, projection,
                         T_camera_world, out, stream);
}

extern "C" int gs_envmap_bwd(int64_t height, int64_t width, int64_t channels, const float* env, int64_t map_edge,
                             const float* weight, int64_t weight_row_stride, int64_t weight_pixel_stride,
                             const float* projection, const float* T_camera_world, const float* grad_out,
                             float* d_weight, float* d_env, void* scratch, int64_t scratch_bytes, void* stream) {
  return env_bwd<float>("gs_envmap_bwd", height, width, channels, env, map_edge, weight, weight_row_stride,
                        weight_pixel_stride, projection, T_camera_world, grad_out, d_weight, d_env, scratch,
                        scratch_bytes, stream);
}

extern "C" int gs_envmap_bwd_f64(int64_t height, int64_t width, int64_t channels, const double* env, int64_t map_edge,
                                 const double* weight, int64_t weight_row_stride, int64_t weight_pixel_stride,
                                 const double* projection, const double* T_camera_world, const double* grad_out,
                                 double* d_weight, double* d_env, void* scratch, int64_t scratch_bytes, void* stream) {
  return env_bwd<double>("gs_envmap_bwd_f64", height, width, channels, env, map_edge, weight, weight_row_stride,
                         weight_pixel_stride, projection, T_camera_world, grad_out, d_weight, d_env, scratch,
                         scratch_bytes, stream);
}
