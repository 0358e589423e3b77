// hg_lab.h -- sRGB <-> normalised CIE Lab, the one statement of the chain that the HG_PROJ_LAB projection of hg_hist.hip and
// the stand-alone conversions of hg_post.hip (hg_srgb_to_lab, hg_lab_to_srgb) evaluate, and -- unrounded, in Lab units -- the
// colour differences of hg_deltae.hip (hg_delta_e).
//
//   c_lin = c / 12.92 (c <= 0.04045), else ((c + 0.055) / 1.055)^2.4
//   (X, Y, Z) = M c_lin, M the D65 matrix below with every row divided by its own sum (so white is (1, 1, 1))
//   f(t) = cbrt(t) (t > (6/29)^3), else t / (3 (6/29)^2) + 4/29
//   L = 116 f(Y) - 16, a = 500 (f(X) - f(Y)), b = 200 (f(Y) - f(Z))
//   (Ln, an, bn) = (L / 100, (a + 128) / 255, (b + 128) / 255)          the 8-bit Lab convention, divided by 255
//
// Everything is evaluated in fp64 on the fp32 inputs and rounded ONCE: an fp32 evaluation moves an by up to 3.8e-7, which
// at sigma = 0.02 moves single kernel values by 2e-5, above the 1e-5 parity bar (the argument project() makes for its three
// fp64 logarithms).  Two fp64 evaluations agree to 1 ulp of the fp32 results.
#pragma once
#include <hip/hip_runtime.h>

namespace hg_lab {

constexpr double kRow0 = 0.412453 + 0.357580 + 0.180423, kRow1 = 0.212671 + 0.715160 + 0.072169,
                 kRow2 = 0.019334 + 0.119193 + 0.950227;
constexpr double kM[3][3] = {{0.412453 / kRow0, 0.357580 / kRow0, 0.180423 / kRow0},
                             {0.212671 / kRow1, 0.715160 / kRow1, 0.072169 / kRow1},
                             {0.019334 / kRow2, 0.119193 / kRow2, 0.950227 / kRow2}};
constexpr double kDelta = 6.0 / 29.0, kDelta3 = kDelta * kDelta * kDelta, kSlope = 1.0 / (3.0 * kDelta * kDelta);
constexpr double kKnee = 0.04045, kKneeLin = kKnee / 12.92;

// inverse of kM by cofactors (compile time)
constexpr double det3(const double (&m)[3][3]) {
  return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
         m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}
constexpr double cof(const double (&m)[3][3], int i, int j) {   // element (i, j) of the inverse times the determinant
  const int r0 = (j + 1) % 3, r1 = (j + 2) % 3, c0 = (i + 1) % 3, c1 = (i + 2) % 3;
  return m[r0][c0] * m[r1][c1] - m[r0][c1] * m[r1][c0];
}
constexpr double kDet = det3(kM);
constexpr double kMi[3][3] = {{cof(kM, 0, 0) / kDet, cof(kM, 0, 1) / kDet, cof(kM, 0, 2) / kDet},
                              {cof(kM, 1, 0) / kDet, cof(kM, 1, 1) / kDet, cof(kM, 1, 2) / kDet},
                              {cof(kM, 2, 0) / kDet, cof(kM, 2, 1) / kDet, cof(kM, 2, 2) / kDet}};

__device__ __forceinline__ double srgb_lin(double c) { return c <= kKnee ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4); }
__device__ __forceinline__ double lab_f(double t) { return t > kDelta3 ? cbrt(t) : t * kSlope + 4.0 / 29.0; }

// sRGB in [0, 1] -> (Ln, an, bn), fp64 rounded once
__device__ __forceinline__ void srgb_to_lab(float r, float g, float b, float &Ln, float &an, float &bn) {
  const double lr = srgb_lin((double)r), lg = srgb_lin((double)g), lb = srgb_lin((double)b);
  const double fx = lab_f(kM[0][0] * lr + kM[0][1] * lg + kM[0][2] * lb);
  const double fy = lab_f(kM[1][0] * lr + kM[1][1] * lg + kM[1][2] * lb);
  const double fz = lab_f(kM[2][0] * lr + kM[2][1] * lg + kM[2][2] * lb);
  Ln = (float)((116.0 * fy - 16.0) / 100.0);
  an = (float)((500.0 * (fx - fy) + 128.0) / 255.0);
  bn = (float)((200.0 * (fy - fz) + 128.0) / 255.0);
}

// (dL/dLn, dL/dan, dL/dbn) -> (dL/dr, dL/dg, dL/db) through the 3x3 Jacobian of srgb_to_lab at (r, g, b).  f is C1 and
// both linear pieces have finite slopes, so this is finite on all of [0, 1]; at a knee the slope is that of the piece the
// forward takes.  f'(t) = f / (3 t) above the knee; (c_lin)' = 2.4 c_lin / (c + 0.055) above its knee: no second pow.
__device__ __forceinline__ void srgb_to_lab_grad(float r, float g, float b, float dLn, float dan, float dbn, float &dr,
                                                 float &dg, float &db) {
  const double c[3] = {(double)r, (double)g, (double)b};
  double lin[3], dlin[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    lin[i] = srgb_lin(c[i]);
    dlin[i] = c[i] <= kKnee ? 1.0 / 12.92 : 2.4 * lin[i] / (c[i] + 0.055);
  }
  double dxyz[3];
  const double dfx = (double)dan * (500.0 / 255.0), dfz = -(double)dbn * (200.0 / 255.0);
  const double df[3] = {dfx, (double)dLn * 1.16 - dfx - dfz, dfz};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double t = kM[i][0] * lin[0] + kM[i][1] * lin[1] + kM[i][2] * lin[2];
    dxyz[i] = df[i] * (t > kDelta3 ? cbrt(t) / (3.0 * t) : kSlope);
  }
  dr = (float)((kM[0][0] * dxyz[0] + kM[1][0] * dxyz[1] + kM[2][0] * dxyz[2]) * dlin[0]);
  dg = (float)((kM[0][1] * dxyz[0] + kM[1][1] * dxyz[1] + kM[2][1] * dxyz[2]) * dlin[1]);
  db = (float)((kM[0][2] * dxyz[0] + kM[1][2] * dxyz[1] + kM[2][2] * dxyz[2]) * dlin[2]);
}

// the exact inverse: (Ln, an, bn) -> sRGB, clipped to [0, 1], fp64 rounded once
__device__ __forceinline__ void lab_to_srgb(float Ln, float an, float bn, float &r, float &g, float &b) {
  const double fy = (100.0 * (double)Ln + 16.0) / 116.0;
  const double fx = fy + (255.0 * (double)an - 128.0) / 500.0, fz = fy - (255.0 * (double)bn - 128.0) / 200.0;
  auto finv = [](double s) { return s > kDelta ? s * s * s : (s - 4.0 / 29.0) / kSlope; };
  const double X = finv(fx), Y = finv(fy), Z = finv(fz);
  auto enc = [](double l) {
    const double c = l <= kKneeLin ? 12.92 * l : 1.055 * pow(l, 1.0 / 2.4) - 0.055;
    return (float)fmin(fmax(c, 0.0), 1.0);
  };
  r = enc(kMi[0][0] * X + kMi[0][1] * Y + kMi[0][2] * Z);
  g = enc(kMi[1][0] * X + kMi[1][1] * Y + kMi[1][2] * Z);
  b = enc(kMi[2][0] * X + kMi[2][1] * Y + kMi[2][2] * Z);
}

// The chain WITHOUT its rounding and without the 8-bit normalisation, for the colour differences of hg_deltae.hip: c (sRGB in
// [0, 1], the fp32 inputs widened) -> lab = (L, a, b) in Lab units, fp64.  With SLOPES it also leaves what lab_pullback needs:
// dlin[j] = (c_lin)'(c_j) and dfp[i] = f'(t_i), the same closed forms as srgb_to_lab_grad (no second pow / cbrt).
template <bool SLOPES>
__device__ __forceinline__ void srgb_to_lab_f64(const double (&c)[3], double (&lab)[3], double (&dlin)[3], double (&dfp)[3]) {
  double lin[3], f[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    lin[j] = srgb_lin(c[j]);
    if constexpr (SLOPES) dlin[j] = c[j] <= kKnee ? 1.0 / 12.92 : 2.4 * lin[j] / (c[j] + 0.055);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double t = kM[i][0] * lin[0] + kM[i][1] * lin[1] + kM[i][2] * lin[2];
    f[i] = lab_f(t);
    if constexpr (SLOPES) dfp[i] = t > kDelta3 ? f[i] / (3.0 * t) : kSlope;
  }
  lab[0] = 116.0 * f[1] - 16.0;
  lab[1] = 500.0 * (f[0] - f[1]);
  lab[2] = 200.0 * (f[1] - f[2]);
}

// The inverse of srgb_to_lab_f64: lab = (L, a, b) in Lab units, fp64 -> sRGB clipped to [0, 1], rounded once.  The same
// pieces as lab_to_srgb, without its fp32 inputs and their 8-bit normalisation (the palette transfer of hg_palette.hip moves
// a pixel in Lab units and comes back through this).
__device__ __forceinline__ void lab_f64_to_srgb(const double (&lab)[3], float (&rgb)[3]) {
  const double fy = (lab[0] + 16.0) / 116.0;
  const double fx = fy + lab[1] / 500.0, fz = fy - lab[2] / 200.0;
  auto finv = [](double s) { return s > kDelta ? s * s * s : (s - 4.0 / 29.0) / kSlope; };
  const double xyz[3] = {finv(fx), finv(fy), finv(fz)};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double l = kMi[i][0] * xyz[0] + kMi[i][1] * xyz[1] + kMi[i][2] * xyz[2];
    const double c = l <= kKneeLin ? 12.92 * l : 1.055 * pow(l, 1.0 / 2.4) - 0.055;
    rgb[i] = (float)fmin(fmax(c, 0.0), 1.0);
  }
}

// (d/dL, d/da, d/db) in Lab units -> (d/dr, d/dg, d/db) through the Jacobian of srgb_to_lab_f64 at the point whose slopes
// dlin, dfp are given; fp64, not rounded.
__device__ __forceinline__ void lab_pullback(const double (&dlin)[3], const double (&dfp)[3], const double (&dlab)[3],
                                             double (&dc)[3]) {
  const double dfx = 500.0 * dlab[1], dfz = -200.0 * dlab[2];
  const double dxyz[3] = {dfx * dfp[0], (116.0 * dlab[0] - dfx - dfz) * dfp[1], dfz * dfp[2]};
#pragma unroll
  for (int j = 0; j < 3; ++j) dc[j] = (kM[0][j] * dxyz[0] + kM[1][j] * dxyz[1] + kM[2][j] * dxyz[2]) * dlin[j];
}

}  // namespace hg_lab
