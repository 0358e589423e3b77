// hg_post.hip -- full-resolution post-processing (include/hg_post.h): the separable MATLAB-style resize, the OpenCV
// pyrDown / pyrUp pair with the Laplacian reconstruction fused into one launch per level, the fp64 colour moments and the
// per-pixel affine of the Monge-Kantorovich colour transfer.  All of that is streaming stencil / reduction work bound by
// HBM bandwidth: one thread per output element, neighbours re-read through L1/L2, no LDS staging.  Bilateral guided
// upsampling adds the fp64 normal equations of its grid fit (per-cell partials, then a gather) and the slice, which
// stages the grid vertices of a pixel tile in LDS.
#include "hg_host.h"
#include "../../include/hg_post.h"
#include "hg_lab.h"

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
    if (clamp_in) v = hg_clamp01(v);
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
__device__ __forceinline__ void block_sum9(double (&s)[MOM_K], double (*sm)[MOM_K]) {   // sm: [4][9] LDS
  const int wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < MOM_K; ++k) {
    s[k] = hg_wave_sum(s[k]);
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
    v = hg_clamp01(v);
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

// ---------------------------------------------------------------------------------------------------------------------
// bilateral guided upsampling.  A pixel p along an axis of n pixels sits at grid coordinate (p + 0.5) (g - 1) / n of an
// axis of g vertices; its floor cell is found in integers, (2p + 1)(g - 1) / (2n), so every kernel and the host agree on
// which cell a pixel belongs to whatever the rounding of the floating-point coordinate.
constexpr int BGU_CHUNK = 256;       // pixels of a cell staged in LDS at a time (one per thread)
constexpr int BGU_PAIRS = 256;       // (corner, corner', j, j') entries of one (z, z') block of a cell's partial
constexpr int BGU_MAX_GD = 64;
constexpr int BGU_MAX_SIDE = 1 << 24;
constexpr int BGU_TILE_ROWS = 4;     // slice tile: one wave per row ...
constexpr int BGU_TILE_GROUPS = 64;  // ... of 64 groups of 4 pixels
constexpr size_t BGU_MAX_LDS = 64 * 1024;

// smallest pixel p >= 0 whose floor cell is >= v, i.e. (2p + 1) g1 >= 2 n v; n when there is none
__host__ __device__ inline int bgu_first_px(int v, int g1, int n) {
  const long long a = 2LL * n * v - g1;
  if (v <= 0 || a <= 0) return 0;
  const long long p = (a + 2LL * g1 - 1) / (2LL * g1);
  return p > n ? n : (int)p;
}

// compensated (Kahan) sum: a cell holds a few hundred pixels, and the result is compared with fp64 products at a few ulp
struct BguSum {
  double s = 0.0, c = 0.0;
  __device__ __forceinline__ void add(double v) {
    const double y = v - c, t = s + y;
    c = (t - s) - y;
    s = t;
  }
};

// Partial normal matrix of one xy floor cell (blockIdx.y, blockIdx.x): thread t = ((ca*4 + cb)*4 + ja)*4 + jb owns the
// entries between corner ca (= dy*2 + dx), channel ja and corner cb, channel jb, for every pair of z vertices at most 1
// apart.  The cell's pixels are walked once per z floor `zs` in row-major order, 256 at a time through LDS, and only
// those whose floor(z) is zs add to the four (zs + a, zs + b) sums -- a fixed order, so repeats are bit-identical.
// P: [cell][z][dz + 1][t], Q: [cell][i][z][c][j] (threads < 48: t = (i*4 + c)*4 + j).
__global__ __launch_bounds__(BGU_CHUNK) void k_bgu_partial(const float *__restrict__ in, const float *__restrict__ out,
                                                            const float *__restrict__ wgt, int h, int w, int gh, int gw,
                                                            int gd, double *__restrict__ P, double *__restrict__ Q) {
  __shared__ double s_w[4][BGU_CHUNK], s_in[4][BGU_CHUNK], s_out[3][BGU_CHUNK], s_fz[BGU_CHUNK], s_wt[BGU_CHUNK];
  __shared__ int s_z0[BGU_CHUNK];
  const int x0 = blockIdx.x, y0 = blockIdx.y, cell = y0 * (gw - 1) + x0, t = threadIdx.x;
  const int xlo = bgu_first_px(x0, gw - 1, w), xhi = bgu_first_px(x0 + 1, gw - 1, w);
  const int ylo = bgu_first_px(y0, gh - 1, h), yhi = bgu_first_px(y0 + 1, gh - 1, h);
  const int rw = xhi - xlo, npx = rw * (yhi - ylo);
  const int jb = t & 3, ja = (t >> 2) & 3, cb = (t >> 4) & 3, ca = t >> 6;
  const int qj = t & 3, qc = (t >> 2) & 3, qi = t >> 4;          // right-hand side, threads < 48
  const size_t hw = (size_t)h * w;
  double *Pc = P + (size_t)cell * gd * 3 * BGU_PAIRS;
  double *Qc = Q + (size_t)cell * 3 * gd * 16;
  double carry = 0.0, qcarry = 0.0;          // the (zs + 1, zs + 1) sums of the previous zs: they belong to vertex zs
  for (int zs = -1; zs < gd; ++zs) {
    BguSum s00, s01, s11, q0, q1;
    for (int base = 0; base < npx; base += BGU_CHUNK) {
      __syncthreads();
      const int p = base + t;
      if (p < npx) {
        const int py = ylo + p / rw, px = xlo + p % rw;
        const size_t o = (size_t)py * w + px;
        const double r = in[o], g = in[hw + o], b = in[2 * hw + o];
        const double fx = (px + 0.5) * (gw - 1) / w - x0, fy = (py + 0.5) * (gh - 1) / h - y0;
        const double cz = (0.25 * r + 0.5 * g + 0.25 * b) * (gd - 1), fl = floor(cz);
        s_z0[t] = !(fl >= -1.0) ? -2 : (fl > (double)gd ? gd : (int)fl);    // outside [-1, gd): no vertex in the grid
        s_fz[t] = cz - fl;
        s_w[0][t] = (1.0 - fy) * (1.0 - fx); s_w[1][t] = (1.0 - fy) * fx;
        s_w[2][t] = fy * (1.0 - fx); s_w[3][t] = fy * fx;
        s_in[0][t] = r; s_in[1][t] = g; s_in[2][t] = b; s_in[3][t] = 1.0;
        s_out[0][t] = out[o]; s_out[1][t] = out[hw + o]; s_out[2][t] = out[2 * hw + o];
        s_wt[t] = wgt ? (double)wgt[o] : 1.0;
      }
      __syncthreads();
      const int n = npx - base < BGU_CHUNK ? npx - base : BGU_CHUNK;
      for (int k = 0; k < n; ++k) {
        if (s_z0[k] != zs) continue;
        const double a1 = s_fz[k], a0 = 1.0 - a1, wt = s_wt[k];
        const double v = wt * s_w[ca][k] * s_w[cb][k] * s_in[ja][k] * s_in[jb][k];
        s00.add(v * a0 * a0); s01.add(v * a0 * a1); s11.add(v * a1 * a1);
        if (t < 48) {
          const double u = wt * s_w[qc][k] * s_in[qj][k] * s_out[qi][k];
          q0.add(u * a0); q1.add(u * a1);
        }
      }
    }
    if (zs >= 0) {
      Pc[(size_t)(zs * 3 + 1) * BGU_PAIRS + t] = carry + s00.s;
      if (zs + 1 < gd) {
        Pc[(size_t)(zs * 3 + 2) * BGU_PAIRS + t] = s01.s;          // (zs, zs + 1)
        Pc[(size_t)((zs + 1) * 3 + 0) * BGU_PAIRS + t] = s01.s;    // (zs + 1, zs): the same product
      }
      if (t < 48) Qc[(size_t)(qi * gd + zs) * 16 + (t & 15)] = qcarry + q0.s;
    }
    carry = s11.s; qcarry = q1.s;
  }
}

// One thread per entry of the slab blocks (diag, then off, then rhs): the up-to-four cells that hold both vertices are
// added in ascending (y0, x0) order; entries between vertices more than 1 apart are written as 0.
__global__ __launch_bounds__(256) void k_bgu_gather(const double *__restrict__ P, const double *__restrict__ Q, int gh,
                                                    int gw, int gd, int slab_y, double *__restrict__ diag,
                                                    double *__restrict__ off, double *__restrict__ rhs) {
  const int S = slab_y ? gh : gw, T = slab_y ? gw : gh, m = T * gd * 4;
  const long long mm = (long long)m * m, nA = (2LL * S - 1) * mm, nB = 3LL * S * m;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= nA + nB) return;
  if (e < nA) {
    const int blk = (int)(e / mm), a = (int)((e % mm) / m), b = (int)(e % m);
    const bool lower = blk >= S;
    const int s = lower ? blk - S : blk, sr = lower ? s + 1 : s;
    const int ja = a & 3, za = (a >> 2) % gd, ta = (a >> 2) / gd, jb = b & 3, zb = (b >> 2) % gd, tb = (b >> 2) / gd;
    const int ya = slab_y ? sr : ta, xa = slab_y ? ta : sr, yb = slab_y ? s : tb, xb = slab_y ? tb : s;
    const int dz = zb - za, dy = ya - yb, dx = xa - xb;
    double v = 0.0;
    if (dz >= -1 && dz <= 1 && dy >= -1 && dy <= 1 && dx >= -1 && dx <= 1) {
      for (int y0 = (ya > yb ? ya : yb) - 1; y0 <= (ya < yb ? ya : yb); ++y0) {
        if (y0 < 0 || y0 > gh - 2) continue;
        for (int x0 = (xa > xb ? xa : xb) - 1; x0 <= (xa < xb ? xa : xb); ++x0) {
          if (x0 < 0 || x0 > gw - 2) continue;
          const int ca = (ya - y0) * 2 + (xa - x0), cb = (yb - y0) * 2 + (xb - x0);
          const size_t cell = (size_t)y0 * (gw - 1) + x0;
          v += P[((cell * gd + za) * 3 + (dz + 1)) * BGU_PAIRS + ((ca * 4 + cb) * 4 + ja) * 4 + jb];
        }
      }
    }
    if (lower) off[e - (long long)S * mm] = v;
    else diag[e] = v;
  } else {
    const long long r = e - nA;
    const int i = (int)(r / ((long long)S * m)), s = (int)((r / m) % S), a = (int)(r % m);
    const int j = a & 3, z = (a >> 2) % gd, tt = (a >> 2) / gd;
    const int y = slab_y ? s : tt, x = slab_y ? tt : s;
    double v = 0.0;
    for (int y0 = y - 1; y0 <= y; ++y0) {
      if (y0 < 0 || y0 > gh - 2) continue;
      for (int x0 = x - 1; x0 <= x; ++x0) {
        if (x0 < 0 || x0 > gw - 2) continue;
        const size_t cell = (size_t)y0 * (gw - 1) + x0;
        v += Q[((cell * 3 + i) * gd + z) * 16 + ((y - y0) * 2 + (x - x0)) * 4 + j];
      }
    }
    rhs[r] = v;
  }
}

// Slice.  A block is 4 waves, one image row each, 64 groups of 4 pixels per row (12 bytes: three dwords).  Groups start
// at the pixel that makes the row's byte address a multiple of 4, so group g of a row covers pixels s + 4 (g - 1) ..,
// s = address & 3, and the partial groups at both ends go byte by byte.  The grid vertices the tile touches are staged
// in LDS, each wave blends them along y for its row, and a pixel then reads 2 (x) x 2 (z) models of 12 floats.
struct BguAxis {
  int v;       // floor cell
  float f;     // fraction
};

__device__ __forceinline__ BguAxis bgu_axis(int p, int g1, int n) {
  const unsigned num = (2u * (unsigned)p + 1u) * (unsigned)g1, den = 2u * (unsigned)n, v = num / den;
  return {(int)v, (float)(num - v * den) / (float)den};
}

__global__ __launch_bounds__(256) void k_bgu_slice(const float *__restrict__ gamma, int gh, int gw, int gd,
                                                   const uint8_t *__restrict__ x, long long xs_h, long long xs_w,
                                                   long long xs_c, void *__restrict__ ov, int out_u8, int H, int W,
                                                   int nyv_cap, int nxv_cap) {
  extern __shared__ __align__(16) float bgu_sm[];
  const int vlen = gd * 12;                                    // floats of one xy vertex
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int px_lo = max(0, (int)blockIdx.x * 256 - 4), px_hi = min(W - 1, (int)blockIdx.x * 256 + 254);
  const int y_lo = blockIdx.y * BGU_TILE_ROWS, y_hi = min(H - 1, y_lo + BGU_TILE_ROWS - 1);
  if (px_lo > px_hi) return;
  const int xv0 = bgu_axis(px_lo, gw - 1, W).v, xv1 = min(gw - 1, bgu_axis(px_hi, gw - 1, W).v + 1);
  const int yv0 = bgu_axis(y_lo, gh - 1, H).v, yv1 = min(gh - 1, bgu_axis(y_hi, gh - 1, H).v + 1);
  const int nxv = xv1 - xv0 + 1, nyv = yv1 - yv0 + 1, rowlen = nxv * vlen;      // nxv <= nxv_cap, nyv <= nyv_cap
  float *patch = bgu_sm, *rows = bgu_sm + (size_t)nyv_cap * nxv_cap * vlen;
  for (int i = threadIdx.x; i < nyv * (rowlen / 4); i += 256) {
    const int yy = i / (rowlen / 4), k = i % (rowlen / 4);
    reinterpret_cast<f32x4 *>(patch + yy * rowlen)[k] =
        reinterpret_cast<const f32x4 *>(gamma + ((size_t)(yv0 + yy) * gw + xv0) * vlen)[k];
  }
  __syncthreads();
  const int y = y_lo + wv;
  float *row = rows + (size_t)wv * nxv_cap * vlen;
  if (y < H) {
    const BguAxis ay = bgu_axis(y, gh - 1, H);
    const f32x4 *p0 = reinterpret_cast<const f32x4 *>(patch + (ay.v - yv0) * rowlen);
    const f32x4 *p1 = reinterpret_cast<const f32x4 *>(patch + (ay.v - yv0 + 1) * rowlen);
    for (int k = lane; k < rowlen / 4; k += 64) reinterpret_cast<f32x4 *>(row)[k] = p0[k] + ay.f * (p1[k] - p0[k]);
  }
  __syncthreads();
  if (y >= H) return;
  const uint8_t *xr = x + (long long)y * xs_h;
  const bool vec_in = xs_w == 3 && xs_c == 1;
  const int s = vec_in ? (int)(reinterpret_cast<uintptr_t>(xr) & 3) : 0;
  const int px0 = s + 4 * ((int)blockIdx.x * BGU_TILE_GROUPS + lane - 1);
  if (px0 + 3 < 0 || px0 >= W) return;
  const bool full = px0 >= 0 && px0 + 3 < W;
  uint8_t rgb[12];
  if (full && vec_in) {
    hg_unpack_rgb4(*reinterpret_cast<const HgBytes12 *>(xr + 3LL * px0), rgb);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int px = px0 + q;
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[q * 3 + c] = px >= 0 && px < W ? xr[(long long)px * xs_w + c * xs_c] : 0;
    }
  }
  float res[12];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int px = min(max(px0 + q, 0), W - 1);
    const BguAxis ax = bgu_axis(px, gw - 1, W);
    const int r = rgb[q * 3], g = rgb[q * 3 + 1], b = rgb[q * 3 + 2];
    const int zn = (r + 2 * g + b) * (gd - 1), zv = zn / 1020, z1 = min(zv + 1, gd - 1);   // luminance 1: fz == 0
    const float fz = (float)(zn - zv * 1020) * (1.f / 1020.f), fx = ax.f;
    const float *c0 = row + (ax.v - xv0) * vlen, *c1 = c0 + vlen;
    const float w00 = (1.f - fx) * (1.f - fz), w01 = (1.f - fx) * fz, w10 = fx * (1.f - fz), w11 = fx * fz;
    const float in[3] = {(float)r * (1.f / 255.f), (float)g * (1.f / 255.f), (float)b * (1.f / 255.f)};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const f32x4 m = w00 * reinterpret_cast<const f32x4 *>(c0 + zv * 12)[i] +
                      w01 * reinterpret_cast<const f32x4 *>(c0 + z1 * 12)[i] +
                      w10 * reinterpret_cast<const f32x4 *>(c1 + zv * 12)[i] +
                      w11 * reinterpret_cast<const f32x4 *>(c1 + z1 * 12)[i];
      res[q * 3 + i] = m[0] * in[0] + m[1] * in[1] + m[2] * in[2] + m[3];
    }
  }
  if (out_u8) {
    uint8_t *orow = static_cast<uint8_t *>(ov) + (size_t)y * W * 3 + 3LL * px0;
    uint8_t q8[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) q8[k] = (uint8_t)floorf(255.f * hg_clamp01(res[k]) + 0.5f);
    if (full && (reinterpret_cast<uintptr_t>(orow) & 3) == 0) {
      *reinterpret_cast<HgBytes12 *>(orow) = hg_pack_rgb4([&](int k) { return q8[k]; });
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (px0 + q >= 0 && px0 + q < W) {
#pragma unroll
          for (int c = 0; c < 3; ++c) orow[q * 3 + c] = q8[q * 3 + c];
        }
    }
  } else {
    float *o = static_cast<float *>(ov);
    const size_t HW = (size_t)H * W;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (px0 + q >= 0 && px0 + q < W) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c * HW + (size_t)y * W + px0 + q] = res[q * 3 + c];
      }
  }
}

// LDS plan of the slice: the most xy vertices a tile can touch (a tile spans <= 259 pixels by 4 rows)
struct BguSlicePlan {
  int nyv, nxv;
  size_t lds;
};

BguSlicePlan bgu_slice_plan(int gh, int gw, int gd, int H, int W) {
  const long long nx = 258LL * (gw - 1) / W + 3, ny = (long long)(BGU_TILE_ROWS - 1) * (gh - 1) / H + 3;
  BguSlicePlan p;
  p.nxv = (int)(nx < gw ? nx : gw);
  p.nyv = (int)(ny < gh ? ny : gh);
  p.lds = (size_t)(p.nyv + BGU_TILE_ROWS) * p.nxv * gd * 12 * sizeof(float);
  return p;
}

bool bgu_grid_args_ok(int gh, int gw, int gd) {
  return gh >= 2 && gw >= 2 && gd >= 2 && gh <= 4096 && gw <= 4096 && gd <= BGU_MAX_GD;
}

// sRGB <-> normalised CIE Lab (hg_lab.h), one pixel per thread; grid = (pixel blocks, B).  x: element strides, out: planar
// contiguous (B, 3, H, W).  TO_LAB clamps its input to [0, 1] first (stage 0 of the histogram blocks).
template <bool TO_LAB>
__global__ __launch_bounds__(256) void k_lab_convert(const float *__restrict__ x, long long xs_b, long long xs_c,
                                                     long long xs_h, long long xs_w, float *__restrict__ out, int H, int W) {
  const long long HW = (long long)H * W, n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= HW) return;
  const int y = (int)(n / W), xx = (int)(n - (long long)y * W);
  const float *px = x + blockIdx.y * xs_b + y * xs_h + xx * xs_w;
  const float c0 = px[0], c1 = px[xs_c], c2 = px[2 * xs_c];
  float o0, o1, o2;
  if constexpr (TO_LAB) hg_lab::srgb_to_lab(hg_clamp01(c0), hg_clamp01(c1), hg_clamp01(c2), o0, o1, o2);
  else hg_lab::lab_to_srgb(c0, c1, c2, o0, o1, o2);
  float *po = out + (long long)blockIdx.y * 3 * HW + n;
  po[0] = o0; po[HW] = o1; po[2 * HW] = o2;
}

template <bool TO_LAB>
int lab_convert(const float *x, int64_t xs_b, int64_t xs_c, int64_t xs_h, int64_t xs_w, float *out, int32_t B, int32_t H,
                int32_t W, void *stream) {
  if (!x || !out || B <= 0 || H <= 0 || W <= 0) return HG_EINVAL;
  const long long nb = ((long long)H * W + 255) / 256;
  if (!grid_ok(nb, B, 1)) return HG_EINVAL;
  return launch(k_lab_convert<TO_LAB>, dim3((unsigned)nb, B), dim3(256), 0, (hipStream_t)stream, x, xs_b, xs_c, xs_h, xs_w, out, H,
                W);
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
  return dispatch([&](auto XU8, auto OU8, auto AXIS) {
    return launch(k_resize_axis<XU8, OU8, AXIS>, grid, dim3(256), 0, (hipStream_t)stream, x, xs_c, xs_h, xs_w, clamp_in, out, os_c,
                  os_h, os_w, Ho, Wo, n_in, weights, indices, taps);
  }, x_u8 != 0, out_u8 != 0, among<0, 1>(axis));
}

int hg_pyr_down(const float *x, float *out, int32_t C, int32_t H, int32_t W, void *stream) {
  if (!x || !out || C <= 0 || H <= 0 || W <= 0) return HG_EINVAL;
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const dim3 grid((Wo + 63) / 64, (Ho + 3) / 4, C);
  if (!grid_ok(grid.x, grid.y, grid.z)) return HG_EINVAL;
  return launch(k_pyr_down, grid, dim3(256), 0, (hipStream_t)stream, x, out, H, W, Ho, Wo);
}

int hg_pyr_up_add(const float *prev, const float *fine_a, const float *coarse_a, float wa, const float *fine_b,
                  const float *coarse_b, float wb, float *out, int32_t C, int32_t h, int32_t w, void *stream) {
  if (!prev || !out || C <= 0 || h <= 0 || w <= 0 || h > (1 << 29) || w > (1 << 29)) return HG_EINVAL;
  if (wa != 0.f && (!fine_a || !coarse_a)) return HG_EINVAL;
  if (wb != 0.f && (!fine_b || !coarse_b)) return HG_EINVAL;
  const dim3 grid((2 * w + 63) / 64, (2 * h + 3) / 4, C);
  if (!grid_ok(grid.x, grid.y, grid.z)) return HG_EINVAL;
  return launch(k_pyr_up_add, grid, dim3(256), 0, (hipStream_t)stream, prev, fine_a, coarse_a, wa, fine_b, coarse_b, wb, out, h, w);
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
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch(k_moments_part, dim3(nb), dim3(MOM_THREADS), 0, st, x, n, pix_stride, chan_stride, part)) return rc;
  return launch(k_moments_finish, dim3(1), dim3(MOM_THREADS), 0, st, part, nb, n, moments);
}

int hg_color_affine(const float *x, int64_t n, int64_t pix_stride, int64_t chan_stride, const float *coef, void *out,
                    int32_t out_u8, void *stream) {
  if (!x || !coef || !out || n <= 0 || pix_stride <= 0 || chan_stride <= 0) return HG_EINVAL;
  AffineCoef k;
  for (int i = 0; i < 15; ++i) k.v[i] = coef[i];
  const long long nb = (n + 255) / 256;
  if (!grid_ok(nb, 1, 1)) return HG_EINVAL;
  return dispatch([&](auto OU8) {
    return launch(k_color_affine<OU8>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, n, pix_stride, chan_stride, k,
                  out);
  }, out_u8 != 0);
}

int hg_u8_hwc_to_f32(const uint8_t *x, float *out, int32_t C, int64_t HW, void *stream) {
  if (!x || !out || C <= 0 || HW <= 0) return HG_EINVAL;
  const long long nb = (HW + 255) / 256;
  if (!grid_ok(nb, C, 1)) return HG_EINVAL;
  return launch(k_u8_hwc_to_f32, dim3((unsigned)nb, C), dim3(256), 0, (hipStream_t)stream, x, out, C, HW);
}

int hg_f32_to_u8_hwc(const float *x, uint8_t *out, int32_t C, int64_t HW, void *stream) {
  if (!x || !out || C <= 0 || HW <= 0) return HG_EINVAL;
  const long long nb = (HW + 255) / 256;
  if (!grid_ok(nb, C, 1)) return HG_EINVAL;
  return launch(k_f32_to_u8_hwc, dim3((unsigned)nb, C), dim3(256), 0, (hipStream_t)stream, x, out, C, HW);
}

size_t hg_bgu_normal_workspace_bytes(int32_t gh, int32_t gw, int32_t gd) {
  if (!bgu_grid_args_ok(gh, gw, gd)) return 0;
  return (size_t)(gh - 1) * (gw - 1) * ((size_t)gd * 3 * BGU_PAIRS + 3 * (size_t)gd * 16) * sizeof(double);
}

int hg_bgu_normal(const float *in_ds, const float *out_ds, const float *weight, int32_t h, int32_t w, int32_t gh,
                  int32_t gw, int32_t gd, double *diag, double *off, double *rhs, void *workspace,
                  size_t workspace_bytes, void *stream) {
  if (!in_ds || !out_ds || !diag || !off || !rhs || !workspace || h <= 0 || w <= 0 || h > BGU_MAX_SIDE ||
      w > BGU_MAX_SIDE || !bgu_grid_args_ok(gh, gw, gd))
    return HG_EINVAL;
  if (workspace_bytes < hg_bgu_normal_workspace_bytes(gh, gw, gd)) return HG_EWORKSPACE;
  if (!grid_ok(gw - 1, gh - 1, 1)) return HG_EINVAL;
  const int slab_y = gh >= gw, S = slab_y ? gh : gw, m = (slab_y ? gw : gh) * gd * 4;
  const long long entries = (2LL * S - 1) * m * m + 3LL * S * m, nb = (entries + 255) / 256;
  if (!grid_ok(nb, 1, 1)) return HG_EINVAL;
  double *P = static_cast<double *>(workspace);
  double *Q = P + (size_t)(gh - 1) * (gw - 1) * gd * 3 * BGU_PAIRS;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch(k_bgu_partial, dim3(gw - 1, gh - 1), dim3(BGU_CHUNK), 0, st, in_ds, out_ds, weight, h, w, gh, gw, gd, P, Q))
    return rc;
  return launch(k_bgu_gather, dim3((unsigned)nb), dim3(256), 0, st, P, Q, gh, gw, gd, slab_y, diag, off, rhs);
}

int hg_bgu_slice(const float *gamma, int32_t gh, int32_t gw, int32_t gd, const uint8_t *photo, int64_t xs_h,
                 int64_t xs_w, int64_t xs_c, void *out, int32_t out_u8, int32_t H, int32_t W, void *stream) {
  if (!gamma || !photo || !out || H <= 0 || W <= 0 || H > BGU_MAX_SIDE || W > BGU_MAX_SIDE ||
      !bgu_grid_args_ok(gh, gw, gd) || (reinterpret_cast<uintptr_t>(gamma) & 15) ||
      (!out_u8 && (reinterpret_cast<uintptr_t>(out) & 3)))
    return HG_EINVAL;
  if (2LL * W * (gw - 1) >= (1LL << 32) || 2LL * H * (gh - 1) >= (1LL << 32)) return HG_EINVAL;   // bgu_axis is 32-bit
  const BguSlicePlan plan = bgu_slice_plan(gh, gw, gd, H, W);
  if (plan.lds > BGU_MAX_LDS) return HG_EUNSUPPORTED;          // a grid finer than the pixels it is sliced at
  const dim3 grid((W + 3) / 4 / BGU_TILE_GROUPS + 1, (H + BGU_TILE_ROWS - 1) / BGU_TILE_ROWS);
  if (!grid_ok(grid.x, grid.y, 1)) return HG_EINVAL;
  // (the one kernel of this file whose dynamic LDS can pass 48 KB: launch asks for it)
  return launch(k_bgu_slice, grid, dim3(256), plan.lds, (hipStream_t)stream, gamma, gh, gw, gd, photo, xs_h, xs_w, xs_c, out,
                out_u8, H, W, plan.nyv, plan.nxv);
}

int hg_srgb_to_lab(const float *x, int64_t xs_b, int64_t xs_c, int64_t xs_h, int64_t xs_w, float *out, int32_t B,
                   int32_t H, int32_t W, void *stream) {
  return lab_convert<true>(x, xs_b, xs_c, xs_h, xs_w, out, B, H, W, stream);
}

int hg_lab_to_srgb(const float *x, int64_t xs_b, int64_t xs_c, int64_t xs_h, int64_t xs_w, float *out, int32_t B,
                   int32_t H, int32_t W, void *stream) {
  return lab_convert<false>(x, xs_b, xs_c, xs_h, xs_w, out, B, H, W, stream);
}

}  // extern "C"
