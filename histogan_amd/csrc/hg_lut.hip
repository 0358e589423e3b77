// hg_lut.hip -- 3D colour lookup tables (include/hg_lut.h, hg_lut_*): a recolouring as a function of colour alone.  A LUT is
// fitted on a pixel-paired 256^2 source / target pair -- the pixels are splatted trilinearly into integer normal sums (64-bit
// counters in LDS where the lattice fits, flushed with integer atomics, so no sum depends on its order), and the displacement
// is smoothed and filled in by red-black Gauss-Seidel sweeps in fp64, one workgroup per channel -- and applied to a photo of
// any size in one memory-bound pass: four pixels per lane, 16-byte accesses, the LUT in LDS up to N = 17.
#include "hg_host.h"
#include "../../include/hg_lut.h"

namespace {

constexpr int LUT_THREADS = 1024;                      // every kernel here: the LDS a workgroup takes leaves room for one or two
constexpr int LUT_TILE = LUT_THREADS * 4;              // apply: pixels of a workgroup per step
constexpr int LUT_APPLY_MAX_BLOCKS = 512;              // two workgroups per CU at N <= 17 (59 KB of LDS each)
constexpr int LUT_APPLY_LDS_N = 17;
constexpr int LUT_SPLAT_LDS_N = 17;                    // 17^3 x 4 x 8 B = 157 216 B of the 160 KiB
constexpr int LUT_SOLVE_LDS_N = 25;                    // 25^3 x 8 B = 125 000 B
constexpr int LUT_SPLAT_SHARE = 4096, LUT_SPLAT_MAX_BLOCKS = 256;
constexpr long long LUT_MAX_PIXELS = 1LL << 22;        // 2^8 2^15 2^17 2^22 = 2^62
constexpr int FB = HG_LUT_COORD_BITS, WB = HG_LUT_WEIGHT_BITS, DB = HG_LUT_DISP_BITS;
constexpr int LUT_ONE = 1 << FB;
static_assert(3 * FB + WB + DB + 1 + 22 <= 62, "the 64-bit sums of 2^22 pixels");
static_assert((size_t)LUT_SPLAT_LDS_N * LUT_SPLAT_LDS_N * LUT_SPLAT_LDS_N * 32 <= 160 * 1024, "the splat's counters");
static_assert((size_t)LUT_SOLVE_LDS_N * LUT_SOLVE_LDS_N * LUT_SOLVE_LDS_N * 8 + LUT_THREADS * 8 <= 160 * 1024, "the solve's lattice");
constexpr int LUT_GRAD_LDS_N = 17;                     // 17^3 x 3 x 8 B = 117 912 B
constexpr int LUT_GRAD_SHARE = 4096, LUT_GRAD_PLAN_BLOCKS = 256, LUT_GRAD_MAX_BLOCKS = 512;
constexpr int LUT_GRAD_BITS = HG_LUT_GRAD_BITS;        // |contribution| <= 2^36 (1 + 2^-17)
constexpr long long LUT_GRAD_MAX_PIXELS = 1LL << 26;   // 2^36 2^26 = 2^62
constexpr size_t LUT_GRAD_HEADER = 16;                 // the workspace: the bits of gmax, then the sums
static_assert(LUT_GRAD_BITS + 26 <= 62, "the 64-bit sums of 2^26 pixels");
static_assert((size_t)LUT_GRAD_LDS_N * LUT_GRAD_LDS_N * LUT_GRAD_LDS_N * 24 <= 160 * 1024, "the backward's counters");

enum { LUT_IN_F32 = 0, LUT_IN_F32_PACKED = 1, LUT_IN_U8 = 2 };

extern __shared__ unsigned long long lut_dyn[];        // apply: the LUT (fp32); splat: the counters; solve: d (fp64)

__device__ __forceinline__ float lut_lerp(float u, float v, float f) { return fmaf(f, v - u, u); }

// v / 255 in fp32, correctly rounded, without the division: the product with the rounded reciprocal and one correction by the
// exact remainder give the quotient's bits for every one of the 256 levels (tests/test_lut_cpu.py checks all of them against
// this sequence; tests/test_lut_gpu.py holds the kernel against the division)
__device__ __forceinline__ float lut_level(uint8_t b) {
  constexpr float r = 1.f / 255.f;
  const float v = (float)b, q = v * r;
  return fmaf(fmaf(-q, 255.f, v), r, q);
}

// one pixel through the LUT at L (LDS or global), clipped to [0, 1]
template <bool TRI>
__device__ __forceinline__ void lut_interp(const float *__restrict__ L, int N, float nm1, const float (&x)[3], float (&o)[3]) {
  int i[3];
  float f[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float xc = hg_clamp01(x[c]);
    i[c] = min((int)(xc * nm1), N - 2);
    f[c] = fmaf(xc, nm1, -(float)i[c]);
  }
  const int sr = 3, sg = 3 * N, sb = 3 * N * N;
  const float *c0 = L + i[2] * sb + i[1] * sg + i[0] * sr;
  if constexpr (TRI) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float e00 = lut_lerp(c0[c], c0[sr + c], f[0]), e10 = lut_lerp(c0[sg + c], c0[sg + sr + c], f[0]);
      const float e01 = lut_lerp(c0[sb + c], c0[sb + sr + c], f[0]), e11 = lut_lerp(c0[sb + sg + c], c0[sb + sg + sr + c], f[0]);
      o[c] = hg_clamp01(lut_lerp(lut_lerp(e00, e10, f[1]), lut_lerp(e01, e11, f[1]), f[2]));
    }
  } else {
    // the axes by descending fraction: steps o1, o2 (the third leads to the opposite corner), fractions a >= b >= c
    int o1, o2;
    float a, b, cc;
    if (f[0] >= f[1]) {
      if (f[1] >= f[2]) { o1 = sr; o2 = sg; a = f[0]; b = f[1]; cc = f[2]; }
      else if (f[0] >= f[2]) { o1 = sr; o2 = sb; a = f[0]; b = f[2]; cc = f[1]; }
      else { o1 = sb; o2 = sr; a = f[2]; b = f[0]; cc = f[1]; }
    } else {
      if (f[2] >= f[1]) { o1 = sb; o2 = sg; a = f[2]; b = f[1]; cc = f[0]; }
      else if (f[2] >= f[0]) { o1 = sg; o2 = sb; a = f[1]; b = f[2]; cc = f[0]; }
      else { o1 = sg; o2 = sr; a = f[1]; b = f[0]; cc = f[2]; }
    }
    const float *c1 = c0 + o1, *c2 = c1 + o2, *c3 = c0 + (sr + sg + sb);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v0 = c0[c], v1 = c1[c], v2 = c2[c], v3 = c3[c];
      o[c] = hg_clamp01(fmaf(cc, v3 - v2, fmaf(b, v2 - v1, fmaf(a, v1 - v0, v0))));
    }
  }
}

template <int IN, bool OU8, bool TRI, bool LDS>
__global__ __launch_bounds__(LUT_THREADS) void k_lut_apply(const void *__restrict__ xv, long long n, long long ps, long long cs,
                                                           const float *__restrict__ lut, int N, void *__restrict__ ov) {
  const float *L = lut;
  if constexpr (LDS) {
    float *stage = reinterpret_cast<float *>(lut_dyn);
    for (int k = threadIdx.x; k < N * N * N * 3; k += LUT_THREADS) stage[k] = lut[k];
    __syncthreads();
    L = stage;
  }
  const float nm1 = (float)(N - 1);
  for (long long tile = blockIdx.x; tile * LUT_TILE < n; tile += gridDim.x) {
    const long long p = tile * LUT_TILE + 4LL * threadIdx.x;
    if (p >= n) break;
    const bool full = p + 3 < n;
    float in[12], res[12];
    if constexpr (IN == LUT_IN_U8) {
      const uint8_t *x = static_cast<const uint8_t *>(xv) + 3 * p;
      uint8_t b8[12];
      if (full) {
        hg_unpack_rgb4(*reinterpret_cast<const HgBytes12 *>(x), b8);
      } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) b8[k] = k < 3 * (int)(n - p) ? x[k] : (uint8_t)0;
      }
#pragma unroll
      for (int k = 0; k < 12; ++k) in[k] = lut_level(b8[k]);
    } else if constexpr (IN == LUT_IN_F32_PACKED) {
      const float *x = static_cast<const float *>(xv) + 3 * p;
      if (full) {
#pragma unroll
        for (int w = 0; w < 3; ++w) {
          const f32x4 v = reinterpret_cast<const f32x4 *>(x)[w];
#pragma unroll
          for (int k = 0; k < 4; ++k) in[4 * w + k] = v[k];
        }
      } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) in[k] = k < 3 * (int)(n - p) ? x[k] : 0.f;
      }
    } else {
      const float *x = static_cast<const float *>(xv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float *px = x + (p + j < n ? p + j : n - 1) * ps;
        in[3 * j] = px[0];
        in[3 * j + 1] = px[cs];
        in[3 * j + 2] = px[2 * cs];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float x3[3] = {in[3 * j], in[3 * j + 1], in[3 * j + 2]};
      float o3[3];
      lut_interp<TRI>(L, N, nm1, x3, o3);
#pragma unroll
      for (int c = 0; c < 3; ++c) res[3 * j + c] = o3[c];
    }
    if constexpr (OU8) {
      uint8_t *o = static_cast<uint8_t *>(ov) + 3 * p;
      uint8_t q8[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) q8[k] = (uint8_t)(res[k] * 255.f);
      if (full) {
        *reinterpret_cast<HgBytes12 *>(o) = hg_pack_rgb4([&](int k) { return q8[k]; });
      } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
          if (k < 3 * (int)(n - p)) o[k] = q8[k];
      }
    } else {
      float *o = static_cast<float *>(ov) + 3 * p;
      if (full) {
#pragma unroll
        for (int w = 0; w < 3; ++w) {
          f32x4 v;
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = res[4 * w + k];
          reinterpret_cast<f32x4 *>(o)[w] = v;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
          if (k < 3 * (int)(n - p)) o[k] = res[k];
      }
    }
  }
}

// the integer normal sums: (A, B_r, B_g, B_b) of the 8 corners of every pixel's cell
template <bool LDS>
__global__ __launch_bounds__(LUT_THREADS) void k_lut_splat(const float *__restrict__ src, long long sps, long long scs,
                                                           const float *__restrict__ tgt, long long tps, long long tcs,
                                                           const float *__restrict__ wt, long long n, int N,
                                                           unsigned long long *__restrict__ sums, long long share) {
  const int n4 = N * N * N * 4;
  unsigned long long *cnt = sums;
  if constexpr (LDS) {
    for (int k = threadIdx.x; k < n4; k += LUT_THREADS) lut_dyn[k] = 0ull;
    __syncthreads();
    cnt = lut_dyn;
  }
  const long long p0 = (long long)blockIdx.x * share, p1 = p0 + share < n ? p0 + share : n;
  for (long long p = p0 + threadIdx.x; p < p1; p += LUT_THREADS) {
    const float *ps = src + p * sps, *pt = tgt + p * tps;
    const float s[3] = {ps[0], ps[scs], ps[2 * scs]}, t[3] = {pt[0], pt[tcs], pt[2 * tcs]};
    const float wv = wt ? wt[p] : 1.f;
    bool ok = isfinite(wv);
#pragma unroll
    for (int c = 0; c < 3; ++c) ok = ok && isfinite(s[c]) && isfinite(t[c]);
    const int qw = ok ? (int)rint((double)hg_clamp01(wv) * (double)(1 << WB)) : 0;
    if (qw == 0) continue;
    int i[3], f[3];
    long long qd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float xc = hg_clamp01(s[c]);
      const int q = (int)rint((double)xc * (double)((N - 1) << FB));
      i[c] = min(q >> FB, N - 2);
      f[c] = q - (i[c] << FB);
      const double d = fmin(fmax((double)t[c] - (double)xc, -2.0), 2.0);
      qd[c] = (long long)rint(d * (double)(1 << DB));
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int jr = j & 1, jg = (j >> 1) & 1, jb = j >> 2;
      const int om = (jr ? f[0] : LUT_ONE - f[0]) * (jg ? f[1] : LUT_ONE - f[1]) * (jb ? f[2] : LUT_ONE - f[2]);
      if (om == 0) continue;                               // also keeps a pixel on the last node inside the lattice
      unsigned long long *c4 = cnt + 4 * (((i[2] + jb) * N + i[1] + jg) * N + i[0] + jr);
      const long long wa = (long long)qw * om;
      atomicAdd(c4, (unsigned long long)wa);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (qd[c] != 0) atomicAdd(c4 + 1 + c, (unsigned long long)(wa * qd[c]));
    }
  }
  if constexpr (LDS) {
    __syncthreads();
    for (int k = threadIdx.x; k < n4; k += LUT_THREADS) {
      const unsigned long long v = lut_dyn[k];
      if (v) atomicAdd(sums + k, v);
    }
  }
}

// (diag(a) + lambda L) d = b for channel blockIdx.x by red-black Gauss-Seidel from d = 0, then LUT = identity + d.  Every
// update is the sequence of roundings include/hg_lut.h states: no contraction into fma.
template <bool LDS>
__global__ __launch_bounds__(LUT_THREADS) void k_lut_solve(const long long *__restrict__ sums, int N, double lambda, int sweeps,
                                                           float *__restrict__ lut, double2 *coef_all, double *d_all) {
#pragma clang fp contract(off)
  __shared__ long long red[LUT_THREADS];
  const int c = blockIdx.x, t = threadIdx.x, n3 = N * N * N;
  long long part = 0;
  for (int k = t; k < n3; k += LUT_THREADS) part += sums[4 * k];
  red[t] = part;
  __syncthreads();
  for (int half = LUT_THREADS / 2; half > 0; half >>= 1) {
    if (t < half) red[t] += red[t + half];
    __syncthreads();
  }
  const long long S = red[0];
  double *d = d_all + (size_t)c * n3;
  if constexpr (LDS) d = reinterpret_cast<double *>(lut_dyn);
  double2 *coef = coef_all + (size_t)c * n3;
  if (S > 0) {
    const double scale = (double)n3 / (double)S;
    for (int k = t; k < n3; k += LUT_THREADS) {
      const int ir = k % N, ig = (k / N) % N, ib = k / (N * N);
      const int deg = (ir > 0) + (ir < N - 1) + (ig > 0) + (ig < N - 1) + (ib > 0) + (ib < N - 1);
      const double a = (double)sums[4 * k] * scale;
      const double b = ((double)sums[4 * k + 1 + c] * scale) * (1.0 / (double)(1 << DB));
      coef[k] = make_double2(b, a + lambda * (double)deg);
      d[k] = 0.0;
    }
    __syncthreads();
    const int H = (N + 1) / 2, units = N * N * H, NN = N * N;
    for (int half = 0; half < 2 * sweeps; ++half) {
      const int colour = half & 1;
      for (int u = t; u < units; u += LUT_THREADS) {
        const int row = u / H, j = u - row * H, ib = row / N, ig = row - ib * N;
        const int ir = 2 * j + ((ib + ig + colour) & 1);
        if (ir >= N) continue;
        const int k = row * N + ir;
        const double2 bc = coef[k];
        if (!(bc.y > 0.0)) continue;                       // lambda == 0 and no data: d stays 0
        double nb = 0.0;
        if (ir > 0) nb += d[k - 1];
        if (ir < N - 1) nb += d[k + 1];
        if (ig > 0) nb += d[k - N];
        if (ig < N - 1) nb += d[k + N];
        if (ib > 0) nb += d[k - NN];
        if (ib < N - 1) nb += d[k + NN];
        d[k] = (bc.x + lambda * nb) / bc.y;
      }
      __syncthreads();
    }
  }
  for (int k = t; k < n3; k += LUT_THREADS) {
    const int ic = c == 0 ? k % N : (c == 1 ? (k / N) % N : k / (N * N));
    const double id = (double)ic / (double)(N - 1);
    lut[3 * (size_t)k + c] = (float)(S > 0 ? id + d[k] : id);
  }
}

// ---- the adjoint of the apply -----------------------------------------------------------------------------------------
// the largest bit pattern of a finite |g|: patterns of non-negative floats order as the floats do
__global__ __launch_bounds__(LUT_THREADS) void k_lut_grad_range(const float *__restrict__ g, long long n3, unsigned *gmax_bits) {
  __shared__ unsigned top;
  if (threadIdx.x == 0) top = 0u;
  __syncthreads();
  unsigned mine = 0u;
  for (long long k = (long long)blockIdx.x * LUT_THREADS + threadIdx.x; k < n3; k += (long long)gridDim.x * LUT_THREADS) {
    const unsigned b = __float_as_uint(g[k]) & 0x7fffffffu;
    if (b < 0x7f800000u && b > mine) mine = b;
  }
  if (mine) atomicMax(&top, mine);
  __syncthreads();
  if (threadIdx.x == 0 && top) atomicMax(gmax_bits, top);
}

// E with gmax < 2^E from the bits of gmax (a subnormal gmax takes E = -126)
__device__ __forceinline__ int lut_grad_exponent(unsigned bits) { return (int)(bits >> 23) - 126; }

// gx and the integer sums of glut for one contiguous share of the pixels per workgroup.  The forward is recomputed with the
// sequence of lut_interp, so the masks are those of the value the forward clipped.
template <bool TRI, bool LDS, bool SUMS>
__global__ __launch_bounds__(LUT_THREADS) void k_lut_apply_bwd(const float *__restrict__ x, long long ps, long long cs,
                                                               const float *__restrict__ lut, int N,
                                                               const float *__restrict__ g, long long n, float *__restrict__ gx,
                                                               const unsigned *__restrict__ gmax_bits,
                                                               unsigned long long *__restrict__ sums, long long share) {
#pragma clang fp contract(off)
  const int n9 = N * N * N * 3;
  unsigned long long *cnt = sums;
  double inv_u = 0.0;
  bool scatter = false;
  if constexpr (SUMS) {
    const unsigned bits = *gmax_bits;
    scatter = bits != 0u;
    inv_u = ldexp(1.0, LUT_GRAD_BITS - lut_grad_exponent(bits));
    if constexpr (LDS) {
      for (int k = threadIdx.x; k < n9; k += LUT_THREADS) lut_dyn[k] = 0ull;
      __syncthreads();
      cnt = lut_dyn;
    }
  }
  const float nm1 = (float)(N - 1);
  const int sr = 3, sg = 3 * N, sb = 3 * N * N;
  const long long p0 = (long long)blockIdx.x * share, p1 = p0 + share < n ? p0 + share : n;
  for (long long p = p0 + threadIdx.x; p < p1; p += LUT_THREADS) {
    const float *px = x + p * ps;
    const float xin[3] = {px[0], px[cs], px[2 * cs]};
    float gm[3];
    int i[3];
    float f[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float gc = g[3 * p + c];
      gm[c] = isfinite(gc) ? gc : 0.f;
      const float xc = hg_clamp01(xin[c]);
      i[c] = min((int)(xc * nm1), N - 2);
      f[c] = fmaf(xc, nm1, -(float)i[c]);
    }
    const int k0 = i[2] * sb + i[1] * sg + i[0] * sr;
    const float *c0 = lut + k0;
    float s[3] = {0.f, 0.f, 0.f};                          // sum over c of m_c g_c (slope of channel c along the axis)
    int node[8];
    double om[8], fd[3];                                   // the weights of the scatter, fp64 from the unrounded fractions
    if constexpr (SUMS) {
#pragma unroll
      for (int c = 0; c < 3; ++c) fd[c] = (double)hg_clamp01(xin[c]) * (double)(N - 1) - (double)i[c];      // exact
    }
    if constexpr (TRI) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v000 = c0[c], v100 = c0[sr + c], v010 = c0[sg + c], v110 = c0[sg + sr + c];
        const float v001 = c0[sb + c], v101 = c0[sb + sr + c], v011 = c0[sb + sg + c], v111 = c0[sb + sg + sr + c];
        const float e00 = lut_lerp(v000, v100, f[0]), e10 = lut_lerp(v010, v110, f[0]);
        const float e01 = lut_lerp(v001, v101, f[0]), e11 = lut_lerp(v011, v111, f[0]);
        const float h0 = lut_lerp(e00, e10, f[1]), h1 = lut_lerp(e01, e11, f[1]);
        const float val = lut_lerp(h0, h1, f[2]);
        if (!(val >= 0.f && val <= 1.f)) gm[c] = 0.f;
        const float dr = lut_lerp(lut_lerp(v100 - v000, v110 - v010, f[1]), lut_lerp(v101 - v001, v111 - v011, f[1]), f[2]);
        const float dg = lut_lerp(e10 - e00, e11 - e01, f[2]);
        const float db = h1 - h0;
        s[0] = fmaf(gm[c], dr, s[0]);
        s[1] = fmaf(gm[c], dg, s[1]);
        s[2] = fmaf(gm[c], db, s[2]);
      }
      if constexpr (SUMS) {
        const double wr[2] = {1.0 - fd[0], fd[0]}, wg[2] = {1.0 - fd[1], fd[1]}, wb[2] = {1.0 - fd[2], fd[2]};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int jr = j & 1, jg = (j >> 1) & 1, jb = j >> 2;
          node[j] = k0 + jr * sr + jg * sg + jb * sb;
          om[j] = (wr[jr] * wg[jg]) * wb[jb];
        }
      }
    } else {
      int o1, o2, a1, a2, a3;                              // steps and axes by descending fraction, as lut_interp sorts them
      float a, b, cc;
      if (f[0] >= f[1]) {
        if (f[1] >= f[2]) { o1 = sr; o2 = sg; a1 = 0; a2 = 1; a3 = 2; a = f[0]; b = f[1]; cc = f[2]; }
        else if (f[0] >= f[2]) { o1 = sr; o2 = sb; a1 = 0; a2 = 2; a3 = 1; a = f[0]; b = f[2]; cc = f[1]; }
        else { o1 = sb; o2 = sr; a1 = 2; a2 = 0; a3 = 1; a = f[2]; b = f[0]; cc = f[1]; }
      } else {
        if (f[2] >= f[1]) { o1 = sb; o2 = sg; a1 = 2; a2 = 1; a3 = 0; a = f[2]; b = f[1]; cc = f[0]; }
        else if (f[2] >= f[0]) { o1 = sg; o2 = sb; a1 = 1; a2 = 2; a3 = 0; a = f[1]; b = f[2]; cc = f[0]; }
        else { o1 = sg; o2 = sr; a1 = 1; a2 = 0; a3 = 2; a = f[1]; b = f[0]; cc = f[2]; }
      }
      const float *c1 = c0 + o1, *c2 = c1 + o2, *c3 = c0 + (sr + sg + sb);
      float t1 = 0.f, t2 = 0.f, t3 = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v0 = c0[c], v1 = c1[c], v2 = c2[c], v3 = c3[c];
        const float val = fmaf(cc, v3 - v2, fmaf(b, v2 - v1, fmaf(a, v1 - v0, v0)));
        if (!(val >= 0.f && val <= 1.f)) gm[c] = 0.f;
        t1 = fmaf(gm[c], v1 - v0, t1);
        t2 = fmaf(gm[c], v2 - v1, t2);
        t3 = fmaf(gm[c], v3 - v2, t3);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] = a1 == c ? t1 : (a2 == c ? t2 : t3);
      if constexpr (SUMS) {
        node[0] = k0; node[1] = k0 + o1; node[2] = k0 + o1 + o2; node[3] = k0 + sr + sg + sb;
        auto along = [&](int ax) { return ax == 0 ? fd[0] : (ax == 1 ? fd[1] : fd[2]); };
        const double ad = along(a1), bd = along(a2), cd = along(a3);
        om[0] = 1.0 - ad; om[1] = ad - bd; om[2] = bd - cd; om[3] = cd;
      }
    }
    if (gx) {
#pragma unroll
      for (int c = 0; c < 3; ++c) gx[3 * p + c] = xin[c] >= 0.f && xin[c] <= 1.f ? nm1 * s[c] : 0.f;
    }
    if constexpr (SUMS) {
      if (scatter) {
        double gs[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) gs[c] = (double)gm[c] * inv_u;             // exact: a power of two
#pragma unroll
        for (int j = 0; j < (TRI ? 8 : 4); ++j) {
          if (om[j] == 0.0) continue;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const long long q = (long long)rint(om[j] * gs[c]);
            if (q != 0) atomicAdd(cnt + node[j] + c, (unsigned long long)q);
          }
        }
      }
    }
  }
  if constexpr (SUMS && LDS) {
    __syncthreads();
    for (int k = threadIdx.x; k < n9; k += LUT_THREADS) {
      const unsigned long long v = lut_dyn[k];
      if (v) atomicAdd(sums + k, v);
    }
  }
}

__global__ __launch_bounds__(256) void k_lut_grad_finish(const long long *__restrict__ sums, const unsigned *__restrict__ gmax_bits,
                                                         int n9, float *__restrict__ glut) {
  const unsigned bits = *gmax_bits;
  const double u = ldexp(1.0, lut_grad_exponent(bits) - LUT_GRAD_BITS);
  for (int k = blockIdx.x * 256 + threadIdx.x; k < n9; k += gridDim.x * 256)
    glut[k] = bits ? (float)((double)sums[k] * u) : 0.f;
}

// gradient of the smoothness term and one Adam step, out of place.  Every line is the sequence include/hg_lut.h states.
__global__ __launch_bounds__(256) void k_lut_adam(const float *__restrict__ lut_in, const float *__restrict__ grad,
                                                  float *__restrict__ m, float *__restrict__ v, float *__restrict__ lut_out, int N,
                                                  float lam_coef, float step_size, float rsbc2, float b1, float b2, float eps) {
#pragma clang fp contract(off)
  const int n9 = N * N * N * 3, NN = N * N;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < n9; e += gridDim.x * 256) {
    const int k = e / 3, c = e - 3 * k;
    const int ir = k % N, ig = (k / N) % N, ib = k / NN;
    float total = grad[e];
    if (lam_coef != 0.f) {
      const float den = (float)(N - 1);
      auto disp = [&](int kk, int jr, int jg, int jb) {
        const int ic = c == 0 ? jr : (c == 1 ? jg : jb);
        return lut_in[3 * kk + c] - (float)((double)ic / (double)den);
      };
      const float d = disp(k, ir, ig, ib);
      float nb = 0.f;
      int deg = 0;
      if (ir > 0) { nb += disp(k - 1, ir - 1, ig, ib); ++deg; }
      if (ir < N - 1) { nb += disp(k + 1, ir + 1, ig, ib); ++deg; }
      if (ig > 0) { nb += disp(k - N, ir, ig - 1, ib); ++deg; }
      if (ig < N - 1) { nb += disp(k + N, ir, ig + 1, ib); ++deg; }
      if (ib > 0) { nb += disp(k - NN, ir, ig, ib - 1); ++deg; }
      if (ib < N - 1) { nb += disp(k + NN, ir, ig, ib + 1); ++deg; }
      total = total + lam_coef * ((float)deg * d - nb);
    }
    const float mi = b1 * m[e] + (1.f - b1) * total;
    const float vi = b2 * v[e] + ((1.f - b2) * total) * total;
    m[e] = mi;
    v[e] = vi;
    lut_out[e] = lut_in[e] - (step_size * mi) / (sqrtf(vi) * rsbc2 + eps);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
size_t lut_up16(size_t v) { return (v + 15) & ~(size_t)15; }
bool lut_aligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }
int lut_check_n(int N) { return N < 2 || N > HG_LUT_MAX_N ? HG_ELUT_SIZE : HG_OK; }

struct LutWorkspace {
  size_t sums, coef, d, total;
};

LutWorkspace lut_workspace(int N) {
  const size_t n3 = (size_t)N * N * N;
  LutWorkspace w;
  size_t o = 0;
  w.sums = o; o += lut_up16(n3 * 4 * sizeof(int64_t));
  w.coef = o; o += lut_up16(3 * n3 * sizeof(double2));
  w.d = o; o += lut_up16(3 * n3 * sizeof(double));
  w.total = o;
  return w;
}

int lut_apply_plan(long long n) {
  const long long b = (n + LUT_TILE - 1) / LUT_TILE;
  return (int)(b < 1 ? 1 : (b > LUT_APPLY_MAX_BLOCKS ? LUT_APPLY_MAX_BLOCKS : b));
}

int lut_splat_plan(long long n) {
  const long long b = (n + LUT_SPLAT_SHARE - 1) / LUT_SPLAT_SHARE;
  return (int)(b < 1 ? 1 : (b > LUT_SPLAT_MAX_BLOCKS ? LUT_SPLAT_MAX_BLOCKS : b));
}

bool lut_pixels_ok(const float *x, long long ps, long long cs) { return x && ps > 0 && cs > 0 && lut_aligned(x, 3); }

int lut_splat(const float *src, long long sps, long long scs, const float *tgt, long long tps, long long tcs, const float *wt,
              long long n, int N, int64_t *sums, int blocks, hipStream_t st) {
  const int nb = blocks > 0 ? blocks : lut_splat_plan(n);
  const long long share = (n + nb - 1) / nb;
  unsigned long long *out = reinterpret_cast<unsigned long long *>(sums);
  return dispatch([&](auto LDS) {
    const size_t lds = LDS ? (size_t)N * N * N * 4 * sizeof(unsigned long long) : 0;
    return launch(k_lut_splat<LDS>, dim3(nb), dim3(LUT_THREADS), lds, st, src, sps, scs, tgt, tps, tcs, wt, n, N, out, share);
  }, N <= LUT_SPLAT_LDS_N);
}

int lut_solve(const int64_t *sums, int N, double lambda, int sweeps, float *lut, char *ws, hipStream_t st) {
  const LutWorkspace w = lut_workspace(N);
  double2 *coef = reinterpret_cast<double2 *>(ws + w.coef);
  double *d = reinterpret_cast<double *>(ws + w.d);
  return dispatch([&](auto LDS) {
    const size_t lds = LDS ? (size_t)N * N * N * sizeof(double) : 0;
    return launch(k_lut_solve<LDS>, dim3(3), dim3(LUT_THREADS), lds, st, reinterpret_cast<const long long *>(sums), N, lambda, sweeps,
                  lut, coef, d);
  }, N <= LUT_SOLVE_LDS_N);
}

bool lut_solver_args_ok(double lambda, int sweeps) { return lambda >= 0.0 && lambda < INFINITY && sweeps >= 0; }

size_t lut_grad_workspace(int N) { return LUT_GRAD_HEADER + lut_up16((size_t)N * N * N * 3 * sizeof(int64_t)); }

int lut_grad_plan(long long n) {
  const long long b = (n + LUT_GRAD_SHARE - 1) / LUT_GRAD_SHARE;
  return (int)(b < 1 ? 1 : (b > LUT_GRAD_PLAN_BLOCKS ? LUT_GRAD_PLAN_BLOCKS : b));
}

bool lut_finite(double v) { return v > -INFINITY && v < INFINITY; }

}  // namespace

extern "C" {

int hg_lut_max_n(void) { return HG_LUT_MAX_N; }
int64_t hg_lut_max_pixels(void) { return LUT_MAX_PIXELS; }
int hg_lut_apply_tile(void) { return LUT_TILE; }
int hg_lut_apply_lds_n(void) { return LUT_APPLY_LDS_N; }
int hg_lut_splat_lds_n(void) { return LUT_SPLAT_LDS_N; }
int hg_lut_solve_lds_n(void) { return LUT_SOLVE_LDS_N; }
int hg_lut_apply_blocks(int64_t n) { return n < 1 ? 0 : lut_apply_plan(n); }
int hg_lut_splat_blocks(int64_t n) { return n < 1 || n > LUT_MAX_PIXELS ? 0 : lut_splat_plan(n); }
size_t hg_lut_workspace_bytes(int32_t N) { return lut_check_n(N) ? 0 : lut_workspace(N).total; }

int hg_lut_apply(const void *x, int32_t x_u8, int64_t n, int64_t pix_stride, int64_t chan_stride, const float *lut, int32_t N,
                 int32_t trilinear, void *out, int32_t out_u8, int32_t blocks, void *stream) {
  if (!x || !lut || !out || n < 1 || blocks < 0 || blocks > LUT_APPLY_MAX_BLOCKS || !lut_aligned(lut, 3) ||
      !lut_aligned(out, out_u8 ? 3 : 15) || !lut_aligned(x, 3))
    return HG_EINVAL;
  if (!x_u8 && (pix_stride <= 0 || chan_stride <= 0)) return HG_EINVAL;
  if (int rc = lut_check_n(N)) return rc;
  const int form = x_u8 ? LUT_IN_U8 : (pix_stride == 3 && chan_stride == 1 && lut_aligned(x, 15) ? LUT_IN_F32_PACKED : LUT_IN_F32);
  const bool lds = N <= LUT_APPLY_LDS_N;
  const size_t lds_bytes = lds ? lut_up16((size_t)N * N * N * 3 * sizeof(float)) : 0;
  const dim3 grid(blocks > 0 ? blocks : lut_apply_plan(n));
  hipStream_t st = (hipStream_t)stream;
  return dispatch([&](auto IN, auto OU8, auto TRI, auto LDS) {
    return launch(k_lut_apply<IN, OU8, TRI, LDS>, grid, dim3(LUT_THREADS), lds_bytes, st, x, n, pix_stride, chan_stride, lut, N, out);
  }, among<LUT_IN_F32, LUT_IN_F32_PACKED, LUT_IN_U8>(form), out_u8 != 0, trilinear != 0, lds);
}

int hg_lut_splat(const float *source, int64_t s_pix_stride, int64_t s_chan_stride, const float *target, int64_t t_pix_stride,
                 int64_t t_chan_stride, const float *weight, int64_t n, int32_t N, int64_t *sums, int32_t blocks, void *stream) {
  if (!lut_pixels_ok(source, s_pix_stride, s_chan_stride) || !lut_pixels_ok(target, t_pix_stride, t_chan_stride) || !sums ||
      !lut_aligned(sums, 7) || !lut_aligned(weight, 3) || n < 1 || blocks < 0 || blocks > LUT_SPLAT_MAX_BLOCKS)
    return HG_EINVAL;
  if (int rc = lut_check_n(N)) return rc;
  if (n > LUT_MAX_PIXELS) return HG_ELUT_PIXELS;
  return lut_splat(source, s_pix_stride, s_chan_stride, target, t_pix_stride, t_chan_stride, weight, n, N, sums, blocks,
                   (hipStream_t)stream);
}

int hg_lut_solve(const int64_t *sums, int32_t N, double lambda, int32_t sweeps, float *lut, void *workspace,
                 size_t workspace_bytes, void *stream) {
  if (!sums || !lut || !workspace || !lut_aligned(sums, 7) || !lut_aligned(lut, 3) || !lut_aligned(workspace, 15) ||
      !lut_solver_args_ok(lambda, sweeps))
    return HG_EINVAL;
  if (int rc = lut_check_n(N)) return rc;
  if (workspace_bytes < lut_workspace(N).total) return HG_EWORKSPACE;
  return lut_solve(sums, N, lambda, sweeps, lut, static_cast<char *>(workspace), (hipStream_t)stream);
}

int hg_lut_fit(const float *source, int64_t s_pix_stride, int64_t s_chan_stride, const float *target, int64_t t_pix_stride,
               int64_t t_chan_stride, const float *weight, int64_t n, int32_t N, double lambda, int32_t sweeps, float *lut,
               void *workspace, size_t workspace_bytes, void *stream) {
  if (!lut_pixels_ok(source, s_pix_stride, s_chan_stride) || !lut_pixels_ok(target, t_pix_stride, t_chan_stride) || !lut ||
      !workspace || !lut_aligned(weight, 3) || !lut_aligned(lut, 3) || !lut_aligned(workspace, 15) || n < 1 ||
      !lut_solver_args_ok(lambda, sweeps))
    return HG_EINVAL;
  if (int rc = lut_check_n(N)) return rc;
  if (n > LUT_MAX_PIXELS) return HG_ELUT_PIXELS;
  const LutWorkspace w = lut_workspace(N);
  if (workspace_bytes < w.total) return HG_EWORKSPACE;
  char *base = static_cast<char *>(workspace);
  int64_t *sums = reinterpret_cast<int64_t *>(base + w.sums);
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(sums, 0, (size_t)N * N * N * 4 * sizeof(int64_t), st);
  if (e != hipSuccess) return (int)e;
  if (int rc = lut_splat(source, s_pix_stride, s_chan_stride, target, t_pix_stride, t_chan_stride, weight, n, N, sums, 0, st))
    return rc;
  return lut_solve(sums, N, lambda, sweeps, lut, base, st);
}

int hg_lut_grad_lds_n(void) { return LUT_GRAD_LDS_N; }
int64_t hg_lut_grad_max_pixels(void) { return LUT_GRAD_MAX_PIXELS; }
int hg_lut_grad_blocks(int64_t n) { return n < 1 || n > LUT_GRAD_MAX_PIXELS ? 0 : lut_grad_plan(n); }
size_t hg_lut_grad_workspace_bytes(int32_t N) { return lut_check_n(N) ? 0 : lut_grad_workspace(N); }

int hg_lut_apply_bwd(const void *x, int32_t x_u8, int64_t n, int64_t pix_stride, int64_t chan_stride, const float *lut, int32_t N,
                     int32_t trilinear, const float *g, float *gx, float *glut, void *workspace, size_t workspace_bytes,
                     int32_t blocks, void *stream) {
  if (x_u8 || !lut_pixels_ok(static_cast<const float *>(x), pix_stride, chan_stride) || !lut || !g || (!gx && !glut) || n < 1 ||
      blocks < 0 || blocks > LUT_GRAD_MAX_BLOCKS || !lut_aligned(lut, 3) || !lut_aligned(g, 3) || !lut_aligned(gx, 3) ||
      !lut_aligned(glut, 3) || (glut && (!workspace || !lut_aligned(workspace, 15))))
    return HG_EINVAL;
  if (int rc = lut_check_n(N)) return rc;
  if (n > LUT_GRAD_MAX_PIXELS) return HG_ELUT_PIXELS;
  if (glut && workspace_bytes < lut_grad_workspace(N)) return HG_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int n9 = N * N * N * 3;
  const int nb = blocks > 0 ? blocks : lut_grad_plan(n);
  const long long share = (n + nb - 1) / nb;
  char *base = static_cast<char *>(workspace);
  unsigned *gmax = reinterpret_cast<unsigned *>(base);
  unsigned long long *sums = glut ? reinterpret_cast<unsigned long long *>(base + LUT_GRAD_HEADER) : nullptr;
  if (glut) {
    const hipError_t e = hipMemsetAsync(base, 0, lut_grad_workspace(N), st);
    if (e != hipSuccess) return (int)e;
    const long long n3 = 3 * (long long)n, rb = (n3 + LUT_THREADS - 1) / LUT_THREADS;
    if (int rc = launch(k_lut_grad_range, dim3((unsigned)(rb > 256 ? 256 : rb)), dim3(LUT_THREADS), 0, st, g, n3, gmax)) return rc;
  }
  const bool lds = glut && N <= LUT_GRAD_LDS_N;
  const size_t lds_bytes = lds ? (size_t)n9 * sizeof(unsigned long long) : 0;
  const int rc = dispatch([&](auto TRI, auto LDS, auto SUMS) {
    if constexpr (decltype(LDS)::value && !decltype(SUMS)::value) return (int)HG_EINVAL;      // never taken: the counters serve the sums
    else
      return launch(k_lut_apply_bwd<TRI, LDS, SUMS>, dim3(nb), dim3(LUT_THREADS), lds_bytes, st, static_cast<const float *>(x),
                    pix_stride, chan_stride, lut, N, g, n, gx, gmax, sums, share);
  }, trilinear != 0, lds, glut != nullptr);
  if (rc || !glut) return rc;
  return launch(k_lut_grad_finish, dim3((n9 + 255) / 256 > 256 ? 256 : (n9 + 255) / 256), dim3(256), 0, st,
                reinterpret_cast<const long long *>(sums), gmax, n9, glut);
}

int hg_lut_adam_step(const float *lut_in, const float *grad, float *exp_avg, float *exp_avg_sq, float *lut_out, int32_t N,
                     double lambda, double lr, double beta1, double beta2, double eps, int32_t step, void *stream) {
  if (!lut_in || !grad || !exp_avg || !exp_avg_sq || !lut_out || lut_in == lut_out || step < 1 || !lut_finite(lr) ||
      !(lambda >= 0.0 && lut_finite(lambda)) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) ||
      !(eps >= 0.0 && lut_finite(eps)) || !lut_aligned(lut_in, 3) || !lut_aligned(grad, 3) || !lut_aligned(exp_avg, 3) ||
      !lut_aligned(exp_avg_sq, 3) || !lut_aligned(lut_out, 3))
    return HG_EINVAL;
  if (int rc = lut_check_n(N)) return rc;
  const double edges = 3.0 * N * N * (N - 1), nm1 = (double)(N - 1);
  const float lam_coef = (float)(lambda * (2.0 * nm1 * nm1 / edges));
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  const float step_size = (float)(lr / bc1), rsbc2 = (float)(1.0 / sqrt(bc2));
  const int n9 = N * N * N * 3, nb = (n9 + 255) / 256;
  return launch(k_lut_adam, dim3(nb > 1024 ? 1024 : nb), dim3(256), 0, (hipStream_t)stream, lut_in, grad, exp_avg, exp_avg_sq,
                lut_out, N, lam_coef, step_size, rsbc2, (float)beta1, (float)beta2, (float)eps);
}

}  // extern "C"
