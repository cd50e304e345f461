// sh_math.h -- the real spherical harmonics of degree 0..3 and their gradient in the direction
// (spherical_harmonics.py:38-106, rsh_cart_0..3), written once over the scalar type: sh.hip instantiates them with float,
// sh_f64.hip with double (gradcheck and the f64 golden values).
#pragma once

#ifdef __HIPCC__
namespace gs_sh {

// A float constant is the decimal rounded to double, then to float; for these twelve that is the float the decimal
// rounds to directly.
template <typename Real> constexpr Real C0v = Real(0.282094791773878);
template <typename Real> constexpr Real C1v = Real(0.48860251190292);
template <typename Real> constexpr Real C2v = Real(1.09254843059208);
template <typename Real> constexpr Real C3v = Real(0.94617469575756);
template <typename Real> constexpr Real C4v = Real(0.31539156525252);
template <typename Real> constexpr Real C5v = Real(0.54627421529604);
template <typename Real> constexpr Real C6v = Real(0.590043589926644);
template <typename Real> constexpr Real C7v = Real(2.89061144264055);
template <typename Real> constexpr Real C8v = Real(0.304697199642977);
template <typename Real> constexpr Real C9v = Real(1.24392110863372);
template <typename Real> constexpr Real C10v = Real(0.497568443453487);
template <typename Real> constexpr Real C11v = Real(1.44530572132028);

template <typename Real, int DEG>
__device__ __forceinline__ void rsh(Real x, Real y, Real z, Real* Y) {
  constexpr Real C1 = C1v<Real>, C2 = C2v<Real>, C3 = C3v<Real>, C4 = C4v<Real>, C5 = C5v<Real>, C6 = C6v<Real>,
                 C7 = C7v<Real>, C8 = C8v<Real>, C9 = C9v<Real>, C10 = C10v<Real>, C11 = C11v<Real>;
  Y[0] = C0v<Real>;
  if (DEG >= 1) { Y[1] = -C1 * y; Y[2] = C1 * z; Y[3] = -C1 * x; }
  if (DEG >= 2) {
    Y[4] = C2 * (x * y); Y[5] = -C2 * (y * z); Y[6] = C3 * (z * z) - C4; Y[7] = -C2 * (x * z);
    Y[8] = C5 * (x * x) - C5 * (y * y);
  }
  if (DEG >= 3) {
    const Real x2 = x * x, y2 = y * y, z2 = z * z;
    Y[9] = -C6 * y * (Real(3) * x2 - y2);
    Y[10] = C7 * (x * y) * z;
    Y[11] = C8 * y * (Real(1.5) - Real(7.5) * z2);
    Y[12] = C9 * z * (Real(1.5) * z2 - Real(0.5)) - C10 * z;
    Y[13] = C8 * x * (Real(1.5) - Real(7.5) * z2);
    Y[14] = C11 * z * (x2 - y2);
    Y[15] = -C6 * x * (x2 - Real(3) * y2);
  }
}

// g_dir = sum_d w[d] * dY_d/d(x,y,z)
template <typename Real, int DEG>
__device__ __forceinline__ void rsh_grad(Real x, Real y, Real z, const Real* w, Real* g) {
  constexpr Real C1 = C1v<Real>, C2 = C2v<Real>, C3 = C3v<Real>, C5 = C5v<Real>, C6 = C6v<Real>, C7 = C7v<Real>,
                 C8 = C8v<Real>, C9 = C9v<Real>, C10 = C10v<Real>, C11 = C11v<Real>;
  g[0] = g[1] = g[2] = Real(0);
  if (DEG >= 1) { g[1] += -C1 * w[1]; g[2] += C1 * w[2]; g[0] += -C1 * w[3]; }
  if (DEG >= 2) {
    g[0] += C2 * y * w[4];            g[1] += C2 * x * w[4];
    g[1] += -C2 * z * w[5];           g[2] += -C2 * y * w[5];
    g[2] += Real(2) * C3 * z * w[6];
    g[0] += -C2 * z * w[7];           g[2] += -C2 * x * w[7];
    g[0] += Real(2) * C5 * x * w[8];  g[1] += Real(-2) * C5 * y * w[8];
  }
  if (DEG >= 3) {
    const Real x2 = x * x, y2 = y * y, z2 = z * z;
    g[0] += Real(-6) * C6 * x * y * w[9];              g[1] += -C6 * (Real(3) * x2 - Real(3) * y2) * w[9];
    g[0] += C7 * y * z * w[10];                        g[1] += C7 * x * z * w[10];    g[2] += C7 * x * y * w[10];
    g[1] += C8 * (Real(1.5) - Real(7.5) * z2) * w[11]; g[2] += Real(-15) * C8 * y * z * w[11];
    g[2] += (C9 * (Real(4.5) * z2 - Real(0.5)) - C10) * w[12];
    g[0] += C8 * (Real(1.5) - Real(7.5) * z2) * w[13]; g[2] += Real(-15) * C8 * x * z * w[13];
    g[0] += Real(2) * C11 * x * z * w[14];             g[1] += Real(-2) * C11 * y * z * w[14];
    g[2] += C11 * (x2 - y2) * w[14];
    g[0] += -C6 * (Real(3) * x2 - Real(3) * y2) * w[15];  g[1] += Real(6) * C6 * x * y * w[15];
  }
}

}  // namespace gs_sh
#endif
