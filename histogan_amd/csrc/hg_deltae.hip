// hg_deltae.hip -- CIE colour difference (dE76, CIEDE2000) between two sRGB images as a fused loss: per-sample weighted mean,
// optional per-pixel map, optional gradient with respect to the first image, in one pass over the pixels.  The definition,
// with its conventions at the singular points, is stated in include/hg_post.h (hg_delta_e); the Lab chain is hg_lab.h's.
//
//   k_de_wsum    (with a map only)  block partials of sum w, fp64, into the workspace
//   k_delta_e    one thread per pixel: both pixels through srgb_to_lab_f64, dE (and its partials with respect to
//                (L1, a1, b1) in forward mode), map / grad written, block partial of sum w dE into the workspace.  With a map
//                every block first sums its sample's partials of sum w (fixed order), because grad needs 1 / sum w.
//   k_de_finish  one block per sample: sums the partials in the same fixed order, mean = sum w dE / sum w
//
// Everything per pixel is fp64 and rounded once; no atomics, so repeats are bit-identical.
#include "hg_host.h"
#include "../../include/hg_post.h"
#include "hg_lab.h"

namespace {

constexpr int DE_THREADS = 256;   // hg_block_sum_256, hg_block_partials_sum_256
constexpr double kDeg = 57.295779513082320877, kRad = 1.0 / kDeg;
constexpr double k25p7 = 6103515625.0;   // 25^7

// ---- forward-mode dual number: a value and N partials (N = 0: the plain value, for the instantiations without grad) -----
template <int N>
struct Dual {
  double v;
  double d[N > 0 ? N : 1];
};

template <int N>
__device__ __forceinline__ Dual<N> cst(double v) {
  Dual<N> r;
  r.v = v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = 0.0;
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> var(double v, int k) {
  Dual<N> r;
  r.v = v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = i == k ? 1.0 : 0.0;
  return r;
}
// r = f(x) with f'(x) = s
template <int N>
__device__ __forceinline__ Dual<N> chain(const Dual<N> &x, double v, double s) {
  Dual<N> r;
  r.v = v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = s * x.d[i];
  return r;
}
// r = f(x, y) with partials sx, sy
template <int N>
__device__ __forceinline__ Dual<N> chain2(const Dual<N> &x, const Dual<N> &y, double v, double sx, double sy) {
  Dual<N> r;
  r.v = v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = sx * x.d[i] + sy * y.d[i];
  return r;
}
template <int N> __device__ __forceinline__ Dual<N> operator+(const Dual<N> &x, const Dual<N> &y) { return chain2(x, y, x.v + y.v, 1.0, 1.0); }
template <int N> __device__ __forceinline__ Dual<N> operator-(const Dual<N> &x, const Dual<N> &y) { return chain2(x, y, x.v - y.v, 1.0, -1.0); }
template <int N> __device__ __forceinline__ Dual<N> operator*(const Dual<N> &x, const Dual<N> &y) { return chain2(x, y, x.v * y.v, y.v, x.v); }
template <int N> __device__ __forceinline__ Dual<N> operator/(const Dual<N> &x, const Dual<N> &y) {
  const double q = x.v / y.v;
  return chain2(x, y, q, 1.0 / y.v, -q / y.v);
}
template <int N> __device__ __forceinline__ Dual<N> operator+(const Dual<N> &x, double c) { return chain(x, x.v + c, 1.0); }
template <int N> __device__ __forceinline__ Dual<N> operator+(double c, const Dual<N> &x) { return chain(x, x.v + c, 1.0); }
template <int N> __device__ __forceinline__ Dual<N> operator-(const Dual<N> &x, double c) { return chain(x, x.v - c, 1.0); }
template <int N> __device__ __forceinline__ Dual<N> operator-(double c, const Dual<N> &x) { return chain(x, c - x.v, -1.0); }
template <int N> __device__ __forceinline__ Dual<N> operator*(const Dual<N> &x, double c) { return chain(x, x.v * c, c); }
template <int N> __device__ __forceinline__ Dual<N> operator*(double c, const Dual<N> &x) { return chain(x, x.v * c, c); }

// the conventions of the definition: a root whose argument is 0 has slope 0, and so has atan2 at the origin
template <int N> __device__ __forceinline__ Dual<N> gsqrt(const Dual<N> &x) {
  const double r = x.v > 0.0 ? sqrt(x.v) : 0.0;
  return chain(x, r, x.v > 0.0 ? 0.5 / r : 0.0);
}
// atan2(y, x) in degrees, mapped into [0, 360); 0 at the origin
template <int N> __device__ __forceinline__ Dual<N> hue(const Dual<N> &y, const Dual<N> &x) {
  const double r2 = x.v * x.v + y.v * y.v;
  const bool origin = x.v == 0.0 && y.v == 0.0;
  double h = origin ? 0.0 : atan2(y.v, x.v) * kDeg;
  h = h < 0.0 ? h + 360.0 : h;
  const double s = origin ? 0.0 : kDeg / r2;
  return chain2(y, x, h, s * x.v, -s * y.v);
}
// cos / sin of an angle in degrees
template <int N> __device__ __forceinline__ Dual<N> dcos(const Dual<N> &x) {
  if constexpr (N > 0) {
    double s, c;
    sincos(x.v * kRad, &s, &c);
    return chain(x, c, -s * kRad);
  } else {
    return chain(x, cos(x.v * kRad), 0.0);
  }
}
template <int N> __device__ __forceinline__ Dual<N> dsin(const Dual<N> &x) {
  if constexpr (N > 0) {
    double s, c;
    sincos(x.v * kRad, &s, &c);
    return chain(x, s, c * kRad);
  } else {
    return chain(x, sin(x.v * kRad), 0.0);
  }
}
template <int N> __device__ __forceinline__ Dual<N> pow7(const Dual<N> &x) {
  const double x2 = x.v * x.v, x6 = x2 * x2 * x2;
  return chain(x, x6 * x.v, 7.0 * x6);
}

// CIEDE2000 (Sharma, Wu, Dalal 2005; kL = kC = kH = 1) of (L1, a1, b1) against the constants (L2, a2, b2): include/hg_post.h
// states every line of it.  N = 3: the partials with respect to (L1, a1, b1) ride along.
template <int N>
__device__ __forceinline__ Dual<N> ciede2000(const double (&p1)[3], const double (&p2)[3]) {
  using D = Dual<N>;
  const D L1 = var<N>(p1[0], 0), a1 = var<N>(p1[1], 1), b1 = var<N>(p1[2], 2);
  const double L2 = p2[0], a2 = p2[1], b2 = p2[2];
  const D C1 = gsqrt(a1 * a1 + b1 * b1);
  const double C2 = sqrt(a2 * a2 + b2 * b2);
  const D Cb7 = pow7((C1 + C2) * 0.5);
  const D G1 = 1.5 - 0.5 * gsqrt(Cb7 / (Cb7 + k25p7));          // 1 + G
  const D a1p = G1 * a1, a2p = G1 * a2;
  const D C1p = gsqrt(a1p * a1p + b1 * b1), C2p = gsqrt(a2p * a2p + b2 * b2);
  const D h1 = hue(b1, a1p), h2 = hue(cst<N>(b2), a2p);
  const bool grey = C1p.v * C2p.v == 0.0;
  // hue difference in (-180, 180], 0 with a grey pixel; mean hue on the same branch
  D dh = h2 - h1;
  if (dh.v > 180.0) dh = dh - 360.0;
  else if (dh.v < -180.0) dh = dh + 360.0;
  D hb = h1 + h2;
  if (grey) {
    dh = cst<N>(0.0);
  } else if (fabs(h1.v - h2.v) <= 180.0) {
    hb = hb * 0.5;
  } else {
    hb = hb.v < 360.0 ? (hb + 360.0) * 0.5 : (hb - 360.0) * 0.5;
  }
  const D dL = L2 - L1, dC = C2p - C1p, dH = 2.0 * (gsqrt(C1p * C2p) * dsin(dh * 0.5));
  const D Lb = (L1 + L2) * 0.5, Cbp = (C1p + C2p) * 0.5;
  const D T = 1.0 - 0.17 * dcos(hb - 30.0) + 0.24 * dcos(hb * 2.0) + 0.32 * dcos(hb * 3.0 + 6.0) - 0.20 * dcos(hb * 4.0 - 63.0);
  const D hq = (hb - 275.0) * (1.0 / 25.0);
  const D hq2 = hq * hq;
  const double ex = 30.0 * exp(-hq2.v);
  const D dtheta = chain(hq2, ex, -ex);
  const D Cbp7 = pow7(Cbp);
  const D RC = 2.0 * gsqrt(Cbp7 / (Cbp7 + k25p7));
  const D l50 = Lb - 50.0;
  const D l2 = l50 * l50;
  const D SL = 1.0 + 0.015 * (l2 / gsqrt(l2 + 20.0)), SC = 1.0 + 0.045 * Cbp, SH = 1.0 + 0.015 * (Cbp * T);
  const D RT = -1.0 * (dsin(dtheta * 2.0) * RC);
  const D tL = dL / SL, tC = dC / SC, tH = dH / SH;
  return gsqrt(tL * tL + tC * tC + tH * tH + RT * (tC * tH));
}

// dE76 and, with N = 3, its partials by hand
template <int N>
__device__ __forceinline__ Dual<N> cie76(const double (&p1)[3], const double (&p2)[3]) {
  const double d0 = p1[0] - p2[0], d1 = p1[1] - p2[1], d2 = p1[2] - p2[2];
  const double q = d0 * d0 + d1 * d1 + d2 * d2;
  Dual<N> r;
  r.v = q > 0.0 ? sqrt(q) : 0.0;
  if constexpr (N > 0) {
    const double inv = q > 0.0 ? 1.0 / r.v : 0.0;
    r.d[0] = d0 * inv;
    r.d[1] = d1 * inv;
    r.d[2] = d2 * inv;
  }
  return r;
}

// grid = (pixel blocks, B).  wpart: the partials of k_de_wsum (weight != NULL).
__global__ __launch_bounds__(DE_THREADS) void k_de_wsum(const float *__restrict__ weight, long long ws_b, long long ws_h,
                                                        long long ws_w, int H, int W, double *__restrict__ wpart) {
  __shared__ double sm4[4];
  const long long HW = (long long)H * W, n = (long long)blockIdx.x * DE_THREADS + threadIdx.x;
  double w = 0.0;
  if (n < HW) {
    const long long y = n / W, x = n - y * W;
    w = (double)hg_clamp01(weight[blockIdx.y * ws_b + y * ws_h + x * ws_w]);
  }
  const double s = hg_block_sum_256(w, sm4);
  if (threadIdx.x == 0) wpart[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

template <int KIND, bool GRAD>
__global__ __launch_bounds__(DE_THREADS) void k_delta_e(const float *__restrict__ x1, long long s1_b, long long s1_c,
                                                        long long s1_h, long long s1_w, const float *__restrict__ x2,
                                                        long long s2_b, long long s2_c, long long s2_h, long long s2_w,
                                                        const float *__restrict__ weight, long long ws_b, long long ws_h,
                                                        long long ws_w, float *__restrict__ map, float *__restrict__ grad,
                                                        int H, int W, double *__restrict__ epart,
                                                        const double *__restrict__ wpart) {
  __shared__ double sm4[4];
  constexpr int N = GRAD ? 3 : 0;
  const long long HW = (long long)H * W, n = (long long)blockIdx.x * DE_THREADS + threadIdx.x;
  const int b = blockIdx.y;
  double inv_sw = 0.0;
  if constexpr (GRAD) {
    const double sw = weight ? hg_block_partials_sum_256(wpart + (size_t)b * gridDim.x, (int)gridDim.x, sm4) : (double)HW;
    inv_sw = sw > 0.0 ? 1.0 / sw : 0.0;
  }
  double we = 0.0;
  if (n < HW) {
    const long long y = n / W, x = n - y * W;
    const float *q1 = x1 + b * s1_b + y * s1_h + x * s1_w, *q2 = x2 + b * s2_b + y * s2_h + x * s2_w;
    const float r1[3] = {q1[0], q1[s1_c], q1[2 * s1_c]};
    const double c1[3] = {(double)hg_clamp01(r1[0]), (double)hg_clamp01(r1[1]), (double)hg_clamp01(r1[2])};
    const double c2[3] = {(double)hg_clamp01(q2[0]), (double)hg_clamp01(q2[s2_c]), (double)hg_clamp01(q2[2 * s2_c])};
    const double w = weight ? (double)hg_clamp01(weight[b * ws_b + y * ws_h + x * ws_w]) : 1.0;
    double p1[3], p2[3], dlin[3], dfp[3], unused0[3], unused1[3];
    hg_lab::srgb_to_lab_f64<GRAD>(c1, p1, dlin, dfp);
    hg_lab::srgb_to_lab_f64<false>(c2, p2, unused0, unused1);
    Dual<N> e;
    if constexpr (KIND == 76) e = cie76<N>(p1, p2);
    else e = ciede2000<N>(p1, p2);
    // equal pixels: dE = 0 with slope 0 by definition.  Stated, not left to the arithmetic: the two inlined copies of the
    // chain need not be contracted into the same fma's, and a last-bit difference of the Lab values would show as 1e-14
    if (c1[0] == c2[0] && c1[1] == c2[1] && c1[2] == c2[2]) e = cst<N>(0.0);
    we = w * e.v;
    if (map) map[(long long)b * HW + n] = (float)e.v;
    if constexpr (GRAD) {
      const double dlab[3] = {e.d[0], e.d[1], e.d[2]};
      double dc[3];
      hg_lab::lab_pullback(dlin, dfp, dlab, dc);
      const double sc = w * inv_sw;
      float *g = grad + (long long)b * 3 * HW + n;
#pragma unroll
      for (int j = 0; j < 3; ++j) g[j * HW] = (r1[j] >= 0.f && r1[j] <= 1.f) ? (float)(sc * dc[j]) : 0.f;   // aten's clamp mask
    }
  }
  const double s = hg_block_sum_256(we, sm4);
  if (threadIdx.x == 0) epart[(size_t)b * gridDim.x + blockIdx.x] = s;
}

// grid = (B): mean[b] = sum w dE / sum w, 0 when sum w = 0
__global__ __launch_bounds__(DE_THREADS) void k_de_finish(const double *__restrict__ epart, const double *__restrict__ wpart,
                                                          int nb, double hw, float *__restrict__ mean) {
  __shared__ double sm4[4];
  const double se = hg_block_partials_sum_256(epart + (size_t)blockIdx.x * nb, nb, sm4);
  const double sw = wpart ? hg_block_partials_sum_256(wpart + (size_t)blockIdx.x * nb, nb, sm4) : hw;
  if (threadIdx.x == 0) mean[blockIdx.x] = sw > 0.0 ? (float)(se / sw) : 0.f;
}

long long de_blocks(int32_t B, int32_t H, int32_t W) {   // pixel blocks per sample; 0 when the sizes or the grid are refused
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  const long long nb = ((long long)H * W + DE_THREADS - 1) / DE_THREADS;
  return grid_ok(nb, B, 1) ? nb : 0;
}

}  // namespace

extern "C" {

size_t hg_delta_e_workspace_bytes(int32_t B, int32_t H, int32_t W) {
  return (size_t)de_blocks(B, H, W) * (size_t)(B > 0 ? B : 0) * 2 * sizeof(double);
}

int hg_delta_e(const float *x1, int64_t s1_b, int64_t s1_c, int64_t s1_h, int64_t s1_w, const float *x2, int64_t s2_b,
               int64_t s2_c, int64_t s2_h, int64_t s2_w, const float *weight, int64_t ws_b, int64_t ws_h, int64_t ws_w,
               int32_t kind, float *mean, float *map, float *grad, int32_t B, int32_t H, int32_t W, void *workspace,
               size_t workspace_bytes, void *stream) {
  if (!x1 || !x2 || !mean || !workspace || (kind != 76 && kind != 2000)) return HG_EINVAL;
  const long long nb = de_blocks(B, H, W);
  if (nb == 0 || workspace_bytes < hg_delta_e_workspace_bytes(B, H, W)) return HG_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  double *epart = static_cast<double *>(workspace), *wpart = weight ? epart + (size_t)B * nb : nullptr;
  const dim3 grid((unsigned)nb, (unsigned)B), block(DE_THREADS);
  if (weight)
    if (int rc = launch(k_de_wsum, grid, block, 0, st, weight, ws_b, ws_h, ws_w, H, W, wpart)) return rc;
  const int rc = dispatch([&](auto KIND, auto GRAD) {
    return launch(k_delta_e<KIND, GRAD>, grid, block, 0, st, x1, s1_b, s1_c, s1_h, s1_w, x2, s2_b, s2_c, s2_h, s2_w, weight, ws_b,
                  ws_h, ws_w, map, grad, H, W, epart, wpart);
  }, among<76, 2000>(kind), grad != nullptr);
  if (rc) return rc;
  return launch(k_de_finish, dim3((unsigned)B), block, 0, st, epart, wpart, (int)nb, (double)H * (double)W, mean);
}

}  // extern "C"
