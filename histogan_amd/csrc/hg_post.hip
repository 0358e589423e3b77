// hg_post.hip -- full-resolution post-processing (include/hg_post.h): the separable MATLAB-style resize, the OpenCV
// pyrDown / pyrUp pair with the Laplacian reconstruction fused into one launch per level, the fp64 colour moments and the
// per-pixel affine of the Monge-Kantorovich colour transfer.  All of it is streaming stencil / reduction work bound by
// HBM bandwidth: one thread per output element, neighbours re-read through L1/L2, no LDS staging.
#include "hg_common.h"
#include "../../include/hg_hist.h"
#include "../../include/hg_post.h"

namespace {

constexpr int MOM_THREADS = 256;
constexpr int MOM_MAX_BLOCKS = 1024;
constexpr int MOM_K = 9;   // s0 s1 s2 s00 s01 s02 s11 s12 s22

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---------------------------------------------------------------------------------------------------------------------
// separable resize along one axis; grid (ceil(Wo/64), ceil(Ho/4), C); (Ho, Wo) is the output extent, n_in the input
// length along the resized axis
template <bool XU8, bool OU8, int AXIS>
__global__ __launch_bounds__(256) void k_resize_axis(const void *__restrict__ xv, long long xs_c, long long xs_h,
                                                     long long xs_w, int clamp_in, void *__restrict__ ov,
                                                     long long os_c, long long os_h, long long os_w, int Ho, int Wo,
                                                     int n_in, const float *__restrict__ wt,
                                                     const int *__restrict__ ind, int taps) {
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6), c = blockIdx.z;
  if (i >= Ho || j >= Wo) return;
  const int o = AXIS == 0 ? i : j;                 // position along the resized axis
  const float *w = wt + (size_t)o * taps;
  const int *id = ind + (size_t)o * taps;
  float acc = 0.f;
  for (int t = 0; t < taps; ++t) {
    const int s = clampi(id[t], 0, n_in - 1);
    const long long off = (long long)c * xs_c + (AXIS == 0 ? (long long)s * xs_h + (long long)j * xs_w
                                                           : (long long)i * xs_h + (long long)s * xs_w);
    float v = XU8 ? (float)static_cast<const uint8_t *>(xv)[off] : static_cast<const float *>(xv)[off];
    if (clamp_in) v = fminf(fmaxf(v, 0.f), 1.f);
    acc += w[t] * v;
  }
  const long long oo = (long long)c * os_c + (long long)i * os_h + (long long)j * os_w;
  if constexpr (OU8) static_cast<uint8_t *>(ov)[oo] = (uint8_t)rintf(fminf(fmaxf(acc, 0.f), 255.f));
  else static_cast<float *>(ov)[oo] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// pyrDown; grid (ceil(Wo/64), ceil(Ho/4), C)
__device__ __forceinline__ int refl101(int p, int n) {   // p in [-2, n+1]
  if (n == 1) return 0;
  p = p < 0 ? -p : p;
  p = p >= n ? 2 * n - 2 - p : p;
  p = p < 0 ? -p : p;                                    // n == 2, p == 3 -> -1 -> 1
  return clampi(p, 0, n - 1);
}

__global__ __launch_bounds__(256) void k_pyr_down(const float *__restrict__ x, float *__restrict__ out, int H, int W,
                                                  int Ho, int Wo) {
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6), c = blockIdx.z;
  if (i >= Ho || j >= Wo) return;
  const float k5[5] = {1.f, 4.f, 6.f, 4.f, 1.f};
  const float *xp = x + (size_t)c * H * W;
  int cols[5];
#pragma unroll
  for (int b = 0; b < 5; ++b) cols[b] = refl101(2 * j + b - 2, W);
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const float *row = xp + (size_t)refl101(2 * i + a - 2, H) * W;
    float r = 0.f;
#pragma unroll
    for (int b = 0; b < 5; ++b) r += k5[b] * row[cols[b]];
    acc += k5[a] * r;
  }
  out[(size_t)c * Ho * Wo + (size_t)i * Wo + j] = acc * (1.f / 256.f);
}

// ---------------------------------------------------------------------------------------------------------------------
// pyrUp taps of output position o along an axis of source length n (weights in eighths)
struct UpTaps {
  int i0, i1, i2;
  float w0, w1, w2;
};

__device__ __forceinline__ UpTaps up_taps(int o, int n) {
  const int i = o >> 1, nx = i + 1 < n ? i + 1 : n - 1;
  UpTaps t;
  if (o & 1) {
    t.i0 = i; t.i1 = nx; t.i2 = i;
    t.w0 = 4.f; t.w1 = 4.f; t.w2 = 0.f;
  } else {
    t.i0 = i > 0 ? i - 1 : (n > 1 ? 1 : 0); t.i1 = i; t.i2 = nx;
    t.w0 = 1.f; t.w1 = 6.f; t.w2 = 1.f;
  }
  return t;
}

__device__ __forceinline__ float up_at(const float *__restrict__ s, int w, const UpTaps &r, const UpTaps &q) {
  const float *r0 = s + (size_t)r.i0 * w, *r1 = s + (size_t)r.i1 * w, *r2 = s + (size_t)r.i2 * w;
  const float a = q.w0 * r0[q.i0] + q.w1 * r0[q.i1] + q.w2 * r0[q.i2];
  const float b = q.w0 * r1[q.i0] + q.w1 * r1[q.i1] + q.w2 * r1[q.i2];
  const float d = q.w0 * r2[q.i0] + q.w1 * r2[q.i1] + q.w2 * r2[q.i2];
  return (r.w0 * a + r.w1 * b + r.w2 * d) * (1.f / 64.f);
}

// grid (ceil(2w/64), ceil(2h/4), C)
__global__ __launch_bounds__(256) void k_pyr_up_add(const float *__restrict__ prev, const float *__restrict__ fa,
                                                    const float *__restrict__ ca, float wa,
                                                    const float *__restrict__ fb, const float *__restrict__ cb,
                                                    float wb, float *__restrict__ out, int h, int w) {
  const int W2 = 2 * w, H2 = 2 * h;
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6), c = blockIdx.z;
  if (i >= H2 || j >= W2) return;
  const UpTaps r = up_taps(i, h), q = up_taps(j, w);
  const size_t cc = (size_t)c * h * w, cf = (size_t)c * H2 * W2, o = cf + (size_t)i * W2 + j;
  float v = up_at(prev + cc, w, r, q);
  if (wa != 0.f) v += wa * (fa[o] - up_at(ca + cc, w, r, q));
  if (wb != 0.f) v += wb * (fb[o] - up_at(cb + cc, w, r, q));
  out[o] = v;
}

// ---------------------------------------------------------------------------------------------------------------------
// colour moments: per-block fp64 partials, then one finishing block; fixed order, so repeats are bit-identical
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void block_sum9(double (&s)[MOM_K], double (*sm)[MOM_K]) {   // sm: [4][9] LDS
  const int wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < MOM_K; ++k) {
    s[k] = wave_sum_d(s[k]);
    if ((threadIdx.x & 63) == 0) sm[wv][k] = s[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < MOM_K; ++k) s[k] = (sm[0][k] + sm[1][k]) + (sm[2][k] + sm[3][k]);
}

int mom_blocks(long long n) {
  const long long b = (n + MOM_THREADS - 1) / MOM_THREADS;
  return (int)(b < MOM_MAX_BLOCKS ? b : MOM_MAX_BLOCKS);
}

__global__ __launch_bounds__(MOM_THREADS) void k_moments_part(const float *__restrict__ x, long long n, long long ps,
                                                              long long cs, double *__restrict__ part) {
  __shared__ double sm[4][MOM_K];
  double s[MOM_K];
#pragma unroll
  for (int k = 0; k < MOM_K; ++k) s[k] = 0.0;
  for (long long p = (long long)blockIdx.x * MOM_THREADS + threadIdx.x; p < n; p += (long long)gridDim.x * MOM_THREADS) {
    const float *px = x + p * ps;
    const double r = px[0], g = px[cs], b = px[2 * cs];
    s[0] += r; s[1] += g; s[2] += b;
    s[3] += r * r; s[4] += r * g; s[5] += r * b;
    s[6] += g * g; s[7] += g * b; s[8] += b * b;
  }
  block_sum9(s, sm);
  if (threadIdx.x < MOM_K) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < MOM_K; ++k) v = threadIdx.x == k ? s[k] : v;
    part[(size_t)blockIdx.x * MOM_K + threadIdx.x] = v;
  }
}

__global__ __launch_bounds__(MOM_THREADS) void k_moments_finish(const double *__restrict__ part, int nb, long long n,
                                                                 double *__restrict__ mom) {
  __shared__ double sm[4][MOM_K];
  double s[MOM_K];
#pragma unroll
  for (int k = 0; k < MOM_K; ++k) s[k] = 0.0;
  for (int b = threadIdx.x; b < nb; b += MOM_THREADS) {
#pragma unroll
    for (int k = 0; k < MOM_K; ++k) s[k] += part[(size_t)b * MOM_K + k];
  }
  block_sum9(s, sm);
  if (threadIdx.x < 12) {
    const double dn = (double)n, m[3] = {s[0] / dn, s[1] / dn, s[2] / dn};
    const int t = threadIdx.x;
    double v;
    if (t < 3) {
      v = m[t];
    } else {
      const int a = (t - 3) / 3, b = (t - 3) % 3, lo = a < b ? a : b, hi = a < b ? b : a;
      const int k = 3 + (lo == 0 ? hi : (lo == 1 ? 2 + hi : 5));   // s00 s01 s02 s11 s12 s22
      double sab = 0.0;
#pragma unroll
      for (int q = 3; q < MOM_K; ++q) sab = q == k ? s[q] : sab;
      double sa = 0.0, sb = 0.0;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        sa = q == a ? s[q] : sa;
        sb = q == b ? s[q] : sb;
      }
      v = (sab - sa * sb / dn) / (dn - 1.0);
    }
    mom[t] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
struct AffineCoef {
  float v[15];   // m0[3], T[9] row-major, m1[3]
};

template <bool OU8>
__global__ __launch_bounds__(256) void k_color_affine(const float *__restrict__ x, long long n, long long ps,
                                                      long long cs, AffineCoef k, void *__restrict__ ov) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const float *px = x + p * ps;
  const float d0 = px[0] - k.v[0], d1 = px[cs] - k.v[1], d2 = px[2 * cs] - k.v[2];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = d0 * k.v[3 + c] + d1 * k.v[6 + c] + d2 * k.v[9 + c] + k.v[12 + c];
    v = fminf(fmaxf(v, 0.f), 1.f);
    if constexpr (OU8) static_cast<uint8_t *>(ov)[p * 3 + c] = (uint8_t)(v * 255.f);
    else static_cast<float *>(ov)[p * 3 + c] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// layout conversions; grid (ceil(HW/256), C)
__global__ __launch_bounds__(256) void k_u8_hwc_to_f32(const uint8_t *__restrict__ x, float *__restrict__ out, int C,
                                                       long long HW) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int c = blockIdx.y;
  out[(long long)c * HW + p] = (float)x[p * C + c] / 255.f;
}

__global__ __launch_bounds__(256) void k_f32_to_u8_hwc(const float *__restrict__ x, uint8_t *__restrict__ out, int C,
                                                       long long HW) {
#pragma clang fp contract(off)
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int c = blockIdx.y;
  float v = x[(long long)c * HW + p] * 255.f;   // torchvision save_image: mul(255), add_(0.5), clamp_(0, 255), to(uint8)
  v = v + 0.5f;
  out[p * C + c] = (uint8_t)fminf(fmaxf(v, 0.f), 255.f);
}

bool grid_ok(long long gx, long long gy, long long gz) {
  return gx >= 1 && gx <= 0x7fffffffLL && gy >= 1 && gy <= 65535 && gz >= 1 && gz <= 65535;
}

}  // namespace

extern "C" {

int hg_resize_axis(const void *x, int32_t x_u8, int64_t xs_c, int64_t xs_h, int64_t xs_w, int32_t clamp_in, void *out,
                   int32_t out_u8, int64_t os_c, int64_t os_h, int64_t os_w, int32_t C, int32_t H, int32_t W,
                   int32_t axis, const float *weights, const int32_t *indices, int32_t out_len, int32_t taps,
                   void *stream) {
  if (!x || !out || !weights || !indices || C <= 0 || H <= 0 || W <= 0 || out_len <= 0 || taps <= 0 ||
      (axis != 0 && axis != 1))
    return HG_EINVAL;
  const int Ho = axis == 0 ? out_len : H, Wo = axis == 0 ? W : out_len, n_in = axis == 0 ? H : W;
  const dim3 grid((Wo + 63) / 64, (Ho + 3) / 4, C);
  if (!grid_ok(grid.x, grid.y, grid.z)) return HG_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const bool xu = x_u8 != 0, ou = out_u8 != 0;
#define HG_RESIZE_LAUNCH(XU, OU, AX)                                                                                   \
  hipLaunchKernelGGL((k_resize_axis<XU, OU, AX>), grid, dim3(256), 0, st, x, (long long)xs_c, (long long)xs_h,         \
                     (long long)xs_w, (int)clamp_in, out, (long long)os_c, (long long)os_h, (long long)os_w, Ho, Wo,  \
                     n_in, weights, indices, (int)taps)
  if (axis == 0) {
    if (xu && ou) HG_RESIZE_LAUNCH(true, true, 0);
    else if (xu) HG_RESIZE_LAUNCH(true, false, 0);
    else if (ou) HG_RESIZE_LAUNCH(false, true, 0);
    else HG_RESIZE_LAUNCH(false, false, 0);
  } else {
    if (xu && ou) HG_RESIZE_LAUNCH(true, true, 1);
    else if (xu) HG_RESIZE_LAUNCH(true, false, 1);
    else if (ou) HG_RESIZE_LAUNCH(false, true, 1);
    else HG_RESIZE_LAUNCH(false, false, 1);
  }
#undef HG_RESIZE_LAUNCH
  HG_LAUNCH_CHECK();
  return HG_OK;
}

int hg_pyr_down(const float *x, float *out, int32_t C, int32_t H, int32_t W, void *stream) {
  if (!x || !out || C <= 0 || H <= 0 || W <= 0) return HG_EINVAL;
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const dim3 grid((Wo + 63) / 64, (Ho + 3) / 4, C);
  if (!grid_ok(grid.x, grid.y, grid.z)) return HG_EINVAL;
  hipLaunchKernelGGL(k_pyr_down, grid, dim3(256), 0, (hipStream_t)stream, x, out, H, W, Ho, Wo);
  HG_LAUNCH_CHECK();
  return HG_OK;
}

int hg_pyr_up_add(const float *prev, const float *fine_a, const float *coarse_a, float wa, const float *fine_b,
                  const float *coarse_b, float wb, float *out, int32_t C, int32_t h, int32_t w, void *stream) {
  if (!prev || !out || C <= 0 || h <= 0 || w <= 0 || h > (1 << 29) || w > (1 << 29)) return HG_EINVAL;
  if (wa != 0.f && (!fine_a || !coarse_a)) return HG_EINVAL;
  if (wb != 0.f && (!fine_b || !coarse_b)) return HG_EINVAL;
  const dim3 grid((2 * w + 63) / 64, (2 * h + 3) / 4, C);
  if (!grid_ok(grid.x, grid.y, grid.z)) return HG_EINVAL;
  hipLaunchKernelGGL(k_pyr_up_add, grid, dim3(256), 0, (hipStream_t)stream, prev, fine_a, coarse_a, wa, fine_b,
                     coarse_b, wb, out, h, w);
  HG_LAUNCH_CHECK();
  return HG_OK;
}

size_t hg_color_moments_workspace_bytes(int64_t n) {
  return n >= 2 ? (size_t)mom_blocks(n) * MOM_K * sizeof(double) : 0;
}

int hg_color_moments(const float *x, int64_t n, int64_t pix_stride, int64_t chan_stride, double *moments,
                     void *workspace, size_t workspace_bytes, void *stream) {
  if (!x || !moments || !workspace || n < 2 || pix_stride <= 0 || chan_stride <= 0) return HG_EINVAL;
  if (workspace_bytes < hg_color_moments_workspace_bytes(n)) return HG_EWORKSPACE;
  const int nb = mom_blocks(n);
  double *part = static_cast<double *>(workspace);
  hipLaunchKernelGGL(k_moments_part, dim3(nb), dim3(MOM_THREADS), 0, (hipStream_t)stream, x, (long long)n,
                     (long long)pix_stride, (long long)chan_stride, part);
  HG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_moments_finish, dim3(1), dim3(MOM_THREADS), 0, (hipStream_t)stream, part, nb, (long long)n,
                     moments);
  HG_LAUNCH_CHECK();
  return HG_OK;
}

int hg_color_affine(const float *x, int64_t n, int64_t pix_stride, int64_t chan_stride, const float *coef, void *out,
                    int32_t out_u8, void *stream) {
  if (!x || !coef || !out || n <= 0 || pix_stride <= 0 || chan_stride <= 0) return HG_EINVAL;
  AffineCoef k;
  for (int i = 0; i < 15; ++i) k.v[i] = coef[i];
  const long long nb = (n + 255) / 256;
  if (!grid_ok(nb, 1, 1)) return HG_EINVAL;
  if (out_u8)
    hipLaunchKernelGGL(k_color_affine<true>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, (long long)n,
                       (long long)pix_stride, (long long)chan_stride, k, out);
  else
    hipLaunchKernelGGL(k_color_affine<false>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, (long long)n,
                       (long long)pix_stride, (long long)chan_stride, k, out);
  HG_LAUNCH_CHECK();
  return HG_OK;
}

int hg_u8_hwc_to_f32(const uint8_t *x, float *out, int32_t C, int64_t HW, void *stream) {
  if (!x || !out || C <= 0 || HW <= 0) return HG_EINVAL;
  const long long nb = (HW + 255) / 256;
  if (!grid_ok(nb, C, 1)) return HG_EINVAL;
  hipLaunchKernelGGL(k_u8_hwc_to_f32, dim3((unsigned)nb, C), dim3(256), 0, (hipStream_t)stream, x, out, C,
                     (long long)HW);
  HG_LAUNCH_CHECK();
  return HG_OK;
}

int hg_f32_to_u8_hwc(const float *x, uint8_t *out, int32_t C, int64_t HW, void *stream) {
  if (!x || !out || C <= 0 || HW <= 0) return HG_EINVAL;
  const long long nb = (HW + 255) / 256;
  if (!grid_ok(nb, C, 1)) return HG_EINVAL;
  hipLaunchKernelGGL(k_f32_to_u8_hwc, dim3((unsigned)nb, C), dim3(256), 0, (hipStream_t)stream, x, out, C,
                     (long long)HW);
  HG_LAUNCH_CHECK();
  return HG_OK;
}

}  // extern "C"
