// hg_ssim.hip -- SSIM of two images as a fused loss and metric, one level per call so that the caller composes MS-SSIM without
// a host read-back.  The definition (planes, window, constants, the three-map gradient) is stated in include/hg_post.h
// (hg_ssim_fwd, hg_ssim_bwd); the Lab chain is hg_lab.h's.
//
//   k_ssim_fwd     one workgroup per 32 x 32 tile of the (H-10) x (W-10) map: both planes of the tile + 10 staged in LDS as
//                  fp64 (sRGB -> L*/100 at load in 'L' mode), the five window means by a separable pass (rows into LDS, then
//                  columns), l, cs, ssim per position; optional map, optional 2x2-pooled fp64 planes for the next level,
//                  block partials of sum ssim and sum cs into the workspace
//   k_ssim_finish  one block per sample: the partials in a fixed order -> (mean ssim, mean cs), fp64
//   k_ssim_bwd     one workgroup per 32 x 32 tile of the INPUT: both planes of the tile + 20 staged, the moments recomputed on
//                  tile + 10, the maps M, Exx, Exy formed from the per-sample coefficients (a, c), the adjoint blur as a
//                  second separable pass over LDS, the coarser level's gradient added, plane gradient (fp64) or final
//                  image gradient (fp32, after the L* pull-back and the clamp's mask) written
//
// Everything per position is fp64 and rounded once; no atomics, so repeats are bit-identical.  The products and sums whose
// exact cancellation makes equal images give ssim = 1 and gradient 0 are written as differences that are 0 term by term
// (l = 1 - (mx - my)^2 / A2, cs = 1 - ((sxx - sxy) + (syy - sxy)) / B2, ...), so that no contraction choice of the compiler
// can break it.
#include <cmath>

#include "hg_host.h"
#include "../../include/hg_post.h"
#include "hg_lab.h"

namespace {

constexpr int T = HG_SSIM_TILE, R = 10, K = 11;      // tile edge, halo, taps
constexpr int THREADS = 256;                         // hg_block_sum_256, hg_block_partials_sum_256
constexpr int FT = T + R;                            // forward: staged edge = 42; backward: edge of the recomputed maps
constexpr int BT = T + 2 * R;                        // backward: staged edge = 52
constexpr int EF = T * T / THREADS;                  // forward: positions per thread = 4 (also the backward's output pixels)
constexpr int EB = (FT * FT + THREADS - 1) / THREADS;   // backward: recomputed positions per thread = 7
constexpr double kC1 = 1e-4, kC2 = 9e-4;
static_assert(T % 2 == 0 && T * T % THREADS == 0 && HG_SSIM_FINISH_THREADS == THREADS, "tile / block shape");

enum { SRC_L = 0, SRC_RGB = 1, SRC_F64 = 2 };   // among<SRC_L, SRC_RGB, SRC_F64>(mode): HG_SSIM_PLANES1 / 3 pick the last
static_assert(SRC_L == HG_SSIM_L && SRC_RGB == HG_SSIM_RGB, "the image modes are their own source kind");

struct Taps {
  double g[K];
};

struct Image {   // fp32 (B, 3, H, W) with element strides, or -- SRC_F64 -- contiguous fp64 (B, planes, H, W)
  const void *p;
  long long sb, sc, sh, sw;
};

// The value exists in a register here: without it the compiler sinks a whole tap chain to its (conditional) use and keeps the
// 11 values it read from LDS alive until then, for every position and quantity at once.
__device__ __forceinline__ void pin(double &v) { asm volatile("" : "+v"(v)); }

// The two plane values of pixel (gy, gx) of sample b, plane pl.  In 'L' mode equal clamped pixels give y = x by construction
// (two inlined copies of the chain need not round alike).  SLOPES ('L' mode, backward): also the raw components of the first
// image and the slopes lab_pullback needs.
template <int SRC, bool SLOPES>
__device__ __forceinline__ void load_pair(const Image &i1, const Image &i2, int b, int pl, int np, int gy, int gx, int H, int W,
                                          double &x, double &y, float (&raw)[3], double (&dlin)[3], double (&dfp)[3]) {
  if constexpr (SRC == SRC_F64) {
    const long long o = (((long long)b * np + pl) * H + gy) * W + gx;
    x = static_cast<const double *>(i1.p)[o];
    y = static_cast<const double *>(i2.p)[o];
  } else if constexpr (SRC == SRC_RGB) {
    raw[0] = static_cast<const float *>(i1.p)[b * i1.sb + pl * i1.sc + gy * i1.sh + gx * i1.sw];
    x = (double)hg_clamp01(raw[0]);
    y = (double)hg_clamp01(static_cast<const float *>(i2.p)[b * i2.sb + pl * i2.sc + gy * i2.sh + gx * i2.sw]);
  } else {
    const float *q1 = static_cast<const float *>(i1.p) + b * i1.sb + gy * i1.sh + gx * i1.sw;
    const float *q2 = static_cast<const float *>(i2.p) + b * i2.sb + gy * i2.sh + gx * i2.sw;
    raw[0] = q1[0], raw[1] = q1[i1.sc], raw[2] = q1[2 * i1.sc];
    const double c1[3] = {(double)hg_clamp01(raw[0]), (double)hg_clamp01(raw[1]), (double)hg_clamp01(raw[2])};
    const double c2[3] = {(double)hg_clamp01(q2[0]), (double)hg_clamp01(q2[i2.sc]), (double)hg_clamp01(q2[2 * i2.sc])};
    double lab[3], u0[3], u1[3];
    hg_lab::srgb_to_lab_f64<SLOPES>(c1, lab, dlin, dfp);
    x = lab[0] / 100.0;
    y = x;
    if (c1[0] != c2[0] || c1[1] != c2[1] || c1[2] != c2[2]) {
      hg_lab::srgb_to_lab_f64<false>(c2, lab, u0, u1);
      y = lab[0] / 100.0;
    }
  }
}

// quantity Q of the five whose window means SSIM needs, at one staged pixel: x, y, xx, yy, xy (rounded products)
template <int Q>
__device__ __forceinline__ double quantity(const double *sx, const double *sy, int o) {
  if constexpr (Q == 0) return sx[o];
  else if constexpr (Q == 1) return sy[o];
  else if constexpr (Q == 2) return sx[o] * sx[o];
  else if constexpr (Q == 3) return sy[o] * sy[o];
  else return sx[o] * sy[o];
}

// Window mean of quantity Q at NE positions per thread.  The staged planes are SE x SE; the row pass leaves SE rows of
// OE = SE - 10 columns in `buf`, the column pass reads them.  Position e of a thread is tid + 256 e, row-major in OE x OE.
// Ends with a barrier, so `buf` is free again.
template <int Q, int SE, int NE>
__device__ __forceinline__ void window_mean(const double *sx, const double *sy, double *buf, const Taps &tp, double (&m)[NE]) {
  constexpr int OE = SE - R;
#pragma unroll 1
  for (int idx = threadIdx.x; idx < SE * OE; idx += THREADS) {
    const int r = idx / OE, c = idx - r * OE;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) s = fma(tp.g[k], quantity<Q>(sx, sy, r * SE + c + k), s);
    buf[idx] = s;
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const int pos = threadIdx.x + e * THREADS;
    double s = 0.0;
    if (pos < OE * OE) {
#pragma unroll
      for (int k = 0; k < K; ++k) s = fma(tp.g[k], buf[pos + k * OE], s);
    }
    pin(s);
    m[e] = s;
    __builtin_amdgcn_sched_barrier(0);   // one position's 11 reads in flight at a time: the registers go to the means
  }
  __syncthreads();
}

struct Stats {   // of one position
  double mx, my, l, cs, a2, b2;
};

// l and cs as 1 minus what separates them from 1: 2 mx my + C1 = A2 - (mx - my)^2 and 2 sxy + C2 = B2 - (sxx + syy - 2 sxy).
// Equal planes give mx == my and exx == eyy == exy bit for bit (the same chain of fma's on the same values), hence exactly 1.
__device__ __forceinline__ Stats stats(double mx, double my, double exx, double eyy, double exy) {
  Stats s;
  s.mx = mx, s.my = my;
  const double sxx = fma(-mx, mx, exx), syy = fma(-my, my, eyy), sxy = fma(-mx, my, exy);
  const double d = mx - my;
  s.a2 = mx * mx + my * my + kC1;
  s.l = 1.0 - d * d / s.a2;
  s.b2 = sxx + syy + kC2;
  s.cs = 1.0 - ((sxx - sxy) + (syy - sxy)) / s.b2;
  return s;
}

// ---- forward -----------------------------------------------------------------------------------------------------------
// grid = (tiles of the map, B).  part: (2, B, tiles) -- sum ssim, then sum cs -- over the tile's positions and the planes.
template <int SRC>
__global__ __launch_bounds__(THREADS) void k_ssim_fwd(Image i1, Image i2, int np, float *__restrict__ map,
                                                      double *__restrict__ pool1, double *__restrict__ pool2, int H, int W,
                                                      int ntx, double *__restrict__ part, Taps tp) {
  __shared__ double sx[FT * FT], sy[FT * FT], buf[FT * T], sm4[4];
  const int b = blockIdx.y, ti = blockIdx.x / ntx, tj = blockIdx.x - ti * ntx;
  const int OH = H - R, OW = W - R, y0 = ti * T, x0 = tj * T;
  const int th = min(T, OH - y0), tw = min(T, OW - x0);              // positions of this tile; th + 10 rows are staged
  const int H2 = H >> 1, W2 = W >> 1;
  // the pooled pixels this tile writes: those of its own 32 rows / columns, and the last tile's run to the image's edge
  const int ph = (y0 + T >= OH ? H2 : (y0 + T) >> 1) - (y0 >> 1), pw = (x0 + T >= OW ? W2 : (x0 + T) >> 1) - (x0 >> 1);
  double sum_s = 0.0, sum_c = 0.0, mp[EF];
#pragma unroll
  for (int e = 0; e < EF; ++e) mp[e] = 0.0;
#pragma unroll 1
  for (int pl = 0; pl < np; ++pl) {
#pragma unroll 1
    for (int idx = threadIdx.x; idx < FT * FT; idx += THREADS) {
      const int r = idx / FT, c = idx - r * FT;
      double x = 0.0, y = 0.0;
      if (r < th + R && c < tw + R) {
        float raw[3];
        double u0[3], u1[3];
        load_pair<SRC, false>(i1, i2, b, pl, np, y0 + r, x0 + c, H, W, x, y, raw, u0, u1);
      }
      sx[idx] = x, sy[idx] = y;
    }
    __syncthreads();
    if (pool1) {
      constexpr int PE = FT / 2;
#pragma unroll 1
      for (int idx = threadIdx.x; idx < PE * PE; idx += THREADS) {
        const int r = idx / PE, c = idx - r * PE;
        if (r < ph && c < pw) {
          const int o = 2 * r * FT + 2 * c;
          const long long d = (((long long)b * np + pl) * H2 + (y0 >> 1) + r) * W2 + (x0 >> 1) + c;
          pool1[d] = 0.25 * ((sx[o] + sx[o + 1]) + (sx[o + FT] + sx[o + FT + 1]));
          pool2[d] = 0.25 * ((sy[o] + sy[o + 1]) + (sy[o + FT] + sy[o + FT + 1]));
        }
      }
    }
    double mx[EF], my[EF], exx[EF], eyy[EF], exy[EF];
    window_mean<0, FT, EF>(sx, sy, buf, tp, mx);
    window_mean<1, FT, EF>(sx, sy, buf, tp, my);
    window_mean<2, FT, EF>(sx, sy, buf, tp, exx);
    window_mean<3, FT, EF>(sx, sy, buf, tp, eyy);
    window_mean<4, FT, EF>(sx, sy, buf, tp, exy);       // (its closing barrier also frees sx, sy for the next plane)
#pragma unroll
    for (int e = 0; e < EF; ++e) {
      const int pos = threadIdx.x + e * THREADS, i = pos / T, j = pos - i * T;
      if (i < th && j < tw) {
        const Stats s = stats(mx[e], my[e], exx[e], eyy[e], exy[e]);
        const double v = s.l * s.cs;
        sum_s += v, sum_c += s.cs, mp[e] += v;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (map) {
#pragma unroll
    for (int e = 0; e < EF; ++e) {
      const int pos = threadIdx.x + e * THREADS, i = pos / T, j = pos - i * T;
      if (i < th && j < tw) map[((long long)b * OH + y0 + i) * OW + x0 + j] = (float)(np == 1 ? mp[e] : mp[e] / (double)np);
    }
  }
  const double bs = hg_block_sum_256(sum_s, sm4), bc = hg_block_sum_256(sum_c, sm4);
  if (threadIdx.x == 0) {
    const size_t nt = gridDim.x, o = (size_t)b * nt + blockIdx.x;
    part[o] = bs;
    part[(size_t)gridDim.y * nt + o] = bc;
  }
}

// grid = (B): means[b] = (sum ssim, sum cs) / n, the partials summed in a fixed order (thread t takes t, t + 256, ...)
__global__ __launch_bounds__(THREADS) void k_ssim_finish(const double *__restrict__ part, int nt, double n,
                                                         double *__restrict__ means) {
  __shared__ double sm4[4];
  for (int q = 0; q < 2; ++q) {
    const double s = hg_block_partials_sum_256(part + ((size_t)q * gridDim.x + blockIdx.x) * nt, nt, sm4);
    if (threadIdx.x == 0) means[2 * blockIdx.x + q] = s / n;
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
// grid = (tiles of the input, B).  coef: (B, 2) = (a_b, c_b).  coarse: the gradient of the pooled planes, (B, np, H/2, W/2),
// or NULL.  grad: fp32 (B, 3, H, W) for SRC_L / SRC_RGB, fp64 (B, np, H, W) for SRC_F64.
template <int SRC>
__global__ __launch_bounds__(THREADS) void k_ssim_bwd(Image i1, Image i2, int np, const double *__restrict__ coef,
                                                      const double *__restrict__ coarse, void *__restrict__ grad, int H, int W,
                                                      int ntx, Taps tp) {
  // stage 1: the planes (2 x 52 x 52) and the row-pass buffer (52 x 42); stage 2, over the same memory: the three maps
  // (3 x 42 x 42) and the adjoint's row-pass buffer (42 x 32)
  constexpr int N1 = 2 * BT * BT + BT * FT, N2 = 3 * FT * FT + FT * T;
  __shared__ double lds[N1 > N2 ? N1 : N2];
  double *sx = lds, *sy = lds + BT * BT, *buf = lds + 2 * BT * BT;
  double *maps = lds, *rb = lds + 3 * FT * FT;
  const int b = blockIdx.y, ti = blockIdx.x / ntx, tj = blockIdx.x - ti * ntx;
  const int OH = H - R, OW = W - R, y0 = ti * T, x0 = tj * T;
  const int H2 = H >> 1, W2 = W >> 1;
  const double inv_n = 1.0 / ((double)OH * (double)OW * (double)np);
  const double a = coef[2 * b] * inv_n, cc = coef[2 * b + 1] * inv_n;
#pragma unroll 1
  for (int pl = 0; pl < np; ++pl) {
    // staged pixel (r, c) is image pixel (y0 - 10 + r, x0 - 10 + c); outside the image: 0 (never used by a valid position)
#pragma unroll 1
    for (int idx = threadIdx.x; idx < BT * BT; idx += THREADS) {
      const int r = idx / BT, c = idx - r * BT, gy = y0 - R + r, gx = x0 - R + c;
      double x = 0.0, y = 0.0;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        float raw[3];
        double u0[3], u1[3];
        load_pair<SRC, false>(i1, i2, b, pl, np, gy, gx, H, W, x, y, raw, u0, u1);
      }
      sx[idx] = x, sy[idx] = y;
    }
    __syncthreads();
    double mx[EB], my[EB], exx[EB], eyy[EB], exy[EB];
    window_mean<0, BT, EB>(sx, sy, buf, tp, mx);
    window_mean<1, BT, EB>(sx, sy, buf, tp, my);
    window_mean<2, BT, EB>(sx, sy, buf, tp, exx);
    window_mean<3, BT, EB>(sx, sy, buf, tp, eyy);
    window_mean<4, BT, EB>(sx, sy, buf, tp, exy);       // (closing barrier: the planes may be overwritten)
    // map position (i, j) is position (y0 - 10 + i, x0 - 10 + j) of the image; the adjoint is zero-padded
#pragma unroll
    for (int e = 0; e < EB; ++e) {
      const int pos = threadIdx.x + e * THREADS;
      if (pos < FT * FT) {
        const int i = pos / FT, j = pos - i * FT, oy = y0 - R + i, ox = x0 - R + j;
        double vM = 0.0, vXX = 0.0, vXY = 0.0;
        if (oy >= 0 && oy < OH && ox >= 0 && ox < OW) {
          const Stats s = stats(mx[e], my[e], exx[e], eyy[e], exy[e]);
          const double q = fma(a, s.l, cc) / s.b2;                 // (a l + c) / B2
          vXY = 2.0 * q;
          vXX = -(q * s.cs);
          const double dl = 2.0 * fma(-s.l, s.mx, s.my) / s.a2;    // dl / dmu_x
          // 2 mx Exx + my Exy = 2 q (my - cs mx): both terms of M are exactly 0 for equal planes
          vM = a * s.cs * dl - 2.0 * q * fma(-s.cs, s.mx, s.my);
        }
        maps[pos] = vM, maps[FT * FT + pos] = vXX, maps[2 * FT * FT + pos] = vXY;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    // adjoint blur of the three maps at the tile's 32 x 32 pixels: pixel (u, v) sums map positions (u + 10 - k, v + 10 - l)
    double g3[3][EF];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const double *mp = maps + m * FT * FT;
#pragma unroll 1
      for (int idx = threadIdx.x; idx < FT * T; idx += THREADS) {
        const int i = idx / T, v = idx - i * T;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) s = fma(tp.g[k], mp[i * FT + v + R - k], s);
        rb[idx] = s;
      }
      __syncthreads();
#pragma unroll
      for (int e = 0; e < EF; ++e) {
        const int pos = threadIdx.x + e * THREADS;      // = u * T + v
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) s = fma(tp.g[k], rb[pos + (R - k) * T], s);
        pin(s);
        g3[m][e] = s;
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();                                  // (the last one also frees the maps for the next plane's staging)
    }
#pragma unroll
    for (int e = 0; e < EF; ++e) {
      const int pos = threadIdx.x + e * THREADS, u = pos / T, v = pos - u * T, gy = y0 + u, gx = x0 + v;
      if (gy < H && gx < W) {
        double x, y, dlin[3], dfp[3];
        float raw[3];
        load_pair<SRC, SRC == SRC_L>(i1, i2, b, pl, np, gy, gx, H, W, x, y, raw, dlin, dfp);
        // 2 x adj(Exx) + y adj(Exy) = y (2 adj(Exx) + adj(Exy)) + 2 (x - y) adj(Exx): for equal planes Exy = -2 Exx bit for
        // bit, the adjoint sums keep that factor, and both terms are exactly 0
        double d = g3[0][e] + (y * (2.0 * g3[1][e] + g3[2][e]) + 2.0 * (x - y) * g3[1][e]);
        if (coarse && (gy >> 1) < H2 && (gx >> 1) < W2)
          d += 0.25 * coarse[(((long long)b * np + pl) * H2 + (gy >> 1)) * W2 + (gx >> 1)];
        if constexpr (SRC == SRC_F64) {
          static_cast<double *>(grad)[(((long long)b * np + pl) * H + gy) * W + gx] = d;
        } else if constexpr (SRC == SRC_RGB) {
          static_cast<float *>(grad)[(((long long)b * 3 + pl) * H + gy) * W + gx] =
              (raw[0] >= 0.f && raw[0] <= 1.f) ? (float)d : 0.f;   // aten's clamp mask
        } else {
          const double dlab[3] = {d / 100.0, 0.0, 0.0};
          double dc[3];
          hg_lab::lab_pullback(dlin, dfp, dlab, dc);
          float *g = static_cast<float *>(grad) + ((long long)b * 3 * H + gy) * W + gx;
#pragma unroll
          for (int j = 0; j < 3; ++j) g[(long long)j * H * W] = (raw[j] >= 0.f && raw[j] <= 1.f) ? (float)dc[j] : 0.f;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------
Taps taps() {   // g_k = exp(-(k - 5)^2 / 4.5) / sum, fp64
  Taps t;
  double s = 0.0;
  for (int k = 0; k < K; ++k) s += t.g[k] = std::exp(-(double)((k - 5) * (k - 5)) / 4.5);
  for (int k = 0; k < K; ++k) t.g[k] /= s;
  return t;
}

int planes_of(int32_t mode) {   // 0 for an unknown mode
  return mode == HG_SSIM_L || mode == HG_SSIM_PLANES1 ? 1 : mode == HG_SSIM_RGB || mode == HG_SSIM_PLANES3 ? 3 : 0;
}

// tiles of an h x w extent; 0 when the sizes or the grid are refused
long long tiles(int32_t B, int32_t H, int32_t W, int32_t h, int32_t w, int *ntx) {
  if (B <= 0 || H < K || W < K) return 0;
  const long long nx = ((long long)w + T - 1) / T, ny = ((long long)h + T - 1) / T;
  *ntx = (int)nx;
  return grid_ok(nx * ny, B, 1) ? nx * ny : 0;
}

}  // namespace

extern "C" {

int hg_ssim_tile(void) { return T; }
int hg_ssim_finish_threads(void) { return THREADS; }

size_t hg_ssim_workspace_bytes(int32_t B, int32_t H, int32_t W) {
  int ntx;
  return (size_t)tiles(B, H, W, H - R, W - R, &ntx) * (size_t)(B > 0 ? B : 0) * 2 * sizeof(double);
}

int hg_ssim_fwd(const void *x1, int64_t s1_b, int64_t s1_c, int64_t s1_h, int64_t s1_w, const void *x2, int64_t s2_b,
                int64_t s2_c, int64_t s2_h, int64_t s2_w, int32_t mode, double *means, float *map, double *pool1,
                double *pool2, int32_t B, int32_t H, int32_t W, void *workspace, size_t workspace_bytes, void *stream) {
  const int np = planes_of(mode);
  if (!x1 || !x2 || !means || !workspace || np == 0 || (pool1 == nullptr) != (pool2 == nullptr)) return HG_EINVAL;
  int ntx = 0;
  const long long nt = tiles(B, H, W, H - R, W - R, &ntx);
  if (nt == 0 || workspace_bytes < hg_ssim_workspace_bytes(B, H, W)) return HG_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const Image i1{x1, s1_b, s1_c, s1_h, s1_w}, i2{x2, s2_b, s2_c, s2_h, s2_w};
  double *part = static_cast<double *>(workspace);
  const int rc = dispatch([&](auto SRC) {
    return launch(k_ssim_fwd<SRC>, dim3((unsigned)nt, (unsigned)B), dim3(THREADS), 0, st, i1, i2, np, map, pool1, pool2, H, W, ntx,
                  part, taps());
  }, among<SRC_L, SRC_RGB, SRC_F64>(mode));
  if (rc) return rc;
  return launch(k_ssim_finish, dim3((unsigned)B), dim3(THREADS), 0, st, part, (int)nt,
                (double)(H - R) * (double)(W - R) * (double)np, means);
}

int hg_ssim_bwd(const void *x1, int64_t s1_b, int64_t s1_c, int64_t s1_h, int64_t s1_w, const void *x2, int64_t s2_b,
                int64_t s2_c, int64_t s2_h, int64_t s2_w, int32_t mode, const double *coef, const double *coarse, void *grad,
                int32_t B, int32_t H, int32_t W, void *stream) {
  const int np = planes_of(mode);
  if (!x1 || !x2 || !coef || !grad || np == 0) return HG_EINVAL;
  int ntx = 0;
  const long long nt = tiles(B, H, W, H, W, &ntx);
  if (nt == 0) return HG_EINVAL;
  const Image i1{x1, s1_b, s1_c, s1_h, s1_w}, i2{x2, s2_b, s2_c, s2_h, s2_w};
  return dispatch([&](auto SRC) {
    return launch(k_ssim_bwd<SRC>, dim3((unsigned)nt, (unsigned)B), dim3(THREADS), 0, (hipStream_t)stream, i1, i2, np, coef, coarse,
                  grad, H, W, ntx, taps());
  }, among<SRC_L, SRC_RGB, SRC_F64>(mode));
}

}  // extern "C"
