// hg_palette.hip -- palette extraction and palette-based colour transfer (include/hg_post.h, hg_palette_*).  An image is
// described by K colours: its pixels become 16-bit integer Lab points, a 16^3 grid of cells seeds K centres by weighted
// farthest-point selection, and a fixed number of Lloyd steps refines them.  Everything that decides the palette is an
// integer: workgroups add into 64-bit LDS counters and flush them to 64-bit global counters, seed scores are compared as
// 128-bit products, and the means are integer floor divisions -- so the result does not depend on the order of any sum and
// repeats are bit-identical.  The transfer moves every pixel in Lab by a smooth blend of the per-cluster shifts, in fp64
// (the rule hg_lab.h argues for), one pass over the image.
#include "hg_host.h"
#include "hg_lab.h"
#include "../../include/hg_post.h"

namespace {

constexpr int PAL_THREADS = 256;             // quantise, step, transfer
constexpr int PAL_WIDE_THREADS = 1024;       // bins and seeds: one workgroup owns all 4096 cells
constexpr int PAL_MAX_K = HG_PALETTE_MAX_K;
constexpr int PAL_SIDE = 16, PAL_CELLS = PAL_SIDE * PAL_SIDE * PAL_SIDE;
constexpr int PAL_CELL_L = 800, PAL_CELL_AB_SHIFT = 11, PAL_AB_OFFSET = 16384;
constexpr int PAL_CELLS_PER_THREAD = PAL_CELLS / PAL_WIDE_THREADS;
constexpr int PAL_COPIES = 16;               // copies of a workgroup's K x 4 LDS counters, by lane & 15: same-address adds of a wave
                                             // drop from 64 to 4
constexpr int PAL_SHARE_PIXELS = 4096;       // the plan gives a workgroup at least this many pixels ...
constexpr int PAL_MAX_BLOCKS = 1024;         // ... and an image at most this many workgroups
constexpr long long PAL_MAX_PIXELS = (1LL << 28) - 1;        // 65535 * 2^15 * (2^28 - 1) < 2^59
constexpr int PAL_MAX_BATCH = 65535;         // a grid dimension
static_assert(PAL_CELLS % PAL_WIDE_THREADS == 0, "every thread of the seed kernel owns the same number of cells");
static_assert(PAL_COPIES * PAL_MAX_K * 4 * sizeof(unsigned long long) <= 16 * 1024, "the step kernel's counters");

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct PalPoint {
  int L, a, b;
  unsigned w;
};

// two points of a 16-byte access: (qL, qa, qb, qw) as four little-endian 16-bit integers each
__device__ __forceinline__ PalPoint pal_unpack(int lo, int hi) {
  PalPoint p;
  p.L = (int)(short)(lo & 0xffff);
  p.a = lo >> 16;
  p.b = (int)(short)(hi & 0xffff);
  p.w = (unsigned)hi >> 16;
  return p;
}

__device__ __forceinline__ void pal_pack(const PalPoint &p, int &lo, int &hi) {
  lo = (p.L & 0xffff) | (int)((unsigned)p.a << 16);
  hi = (p.b & 0xffff) | (int)(p.w << 16);
}

__device__ __forceinline__ int pal_cell(const PalPoint &p) {
  const int bL = min(max(p.L, 0) / PAL_CELL_L, PAL_SIDE - 1);
  const int ba = min(max((p.a + PAL_AB_OFFSET) >> PAL_CELL_AB_SHIFT, 0), PAL_SIDE - 1);
  const int bb = min(max((p.b + PAL_AB_OFFSET) >> PAL_CELL_AB_SHIFT, 0), PAL_SIDE - 1);
  return (bL * PAL_SIDE + ba) * PAL_SIDE + bb;
}

// squared distance of two points whose coordinates fit 16 bits: three 32 x 32 + 64 multiply-adds, exact
__device__ __forceinline__ unsigned long long pal_d2(int L0, int a0, int b0, int L1, int a1, int b1) {
  const unsigned dL = (unsigned)abs(L0 - L1), da = (unsigned)abs(a0 - a1), db = (unsigned)abs(b0 - b1);
  return (unsigned long long)dL * dL + (unsigned long long)da * da + (unsigned long long)db * db;
}

// floor((2 S + W) / (2 W)) for W > 0: the mean rounded to nearest, halves up
__device__ __forceinline__ int pal_mean(long long S, long long W) {
  const long long num = 2 * S + W, den = 2 * W;
  long long q = num / den;
  if (num % den != 0 && num < 0) --q;
  return (int)q;
}

struct U128 {
  unsigned long long hi, lo;
};
__device__ __forceinline__ U128 mul128(unsigned long long a, unsigned long long b) { return {__umul64hi(a, b), a * b}; }

// a seed candidate: the larger score wins, the lower cell index on ties
struct PalBest {
  unsigned long long hi, lo;
  int cell;
};
__device__ __forceinline__ bool pal_better(const PalBest &a, const PalBest &b) {
  if (a.hi != b.hi) return a.hi > b.hi;
  if (a.lo != b.lo) return a.lo > b.lo;
  return a.cell < b.cell;
}

struct PalShare {
  int blocks;
  long long share;  // pixels of a workgroup, % 2 == 0
};

int pal_plan_blocks(long long n) {
  const long long b = (n + PAL_SHARE_PIXELS - 1) / PAL_SHARE_PIXELS;
  return (int)(b < 1 ? 1 : (b > PAL_MAX_BLOCKS ? PAL_MAX_BLOCKS : b));
}

PalShare pal_share(long long n, int blocks) {
  PalShare s;
  s.blocks = blocks > 0 ? blocks : pal_plan_blocks(n);
  s.share = ((n + s.blocks - 1) / s.blocks + 1) & ~1LL;
  return s;
}

long long pal_stride(long long n) { return (n + 1) & ~1LL; }

// ---------------------------------------------------------------------------------------------------------------------
// pixels -> points, two per lane and 16-byte store; the points past n up to the stride are written as qw = 0
__global__ __launch_bounds__(PAL_THREADS) void k_pal_quantize(const float *__restrict__ x, long long xs_b, long long xs_c,
                                                              long long xs_h, long long xs_w, const float *__restrict__ wt,
                                                              long long ws_b, long long ws_h, long long ws_w,
                                                              i32x4 *__restrict__ points, long long n, long long stride, int W) {
  const long long pair = (long long)blockIdx.x * PAL_THREADS + threadIdx.x;
  if (2 * pair >= stride) return;
  const int b = blockIdx.y;
  int packed[4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const long long p = 2 * pair + j;
    PalPoint q = {0, 0, 0, 0u};
    if (p < n) {
      const long long h = p / W, w = p - h * W;
      const float *px = x + b * xs_b + h * xs_h + w * xs_w;
      const float c0 = px[0], c1 = px[xs_c], c2 = px[2 * xs_c];
      const float wv = wt ? wt[b * ws_b + h * ws_h + w * ws_w] : 1.f;
      if (isfinite(c0) && isfinite(c1) && isfinite(c2) && isfinite(wv)) {
        const double c[3] = {(double)hg_clamp01(c0), (double)hg_clamp01(c1), (double)hg_clamp01(c2)};
        double lab[3], unused0[3], unused1[3];
        hg_lab::srgb_to_lab_f64<false>(c, lab, unused0, unused1);
        q.L = (int)rint(128.0 * lab[0]);
        q.a = (int)rint(128.0 * lab[1]);
        q.b = (int)rint(128.0 * lab[2]);
        q.w = (unsigned)rint(65535.0 * (double)hg_clamp01(wv));
      }
    }
    pal_pack(q, packed[2 * j], packed[2 * j + 1]);
  }
  points[b * (stride / 2) + pair] = i32x4{packed[0], packed[1], packed[2], packed[3]};
}

// W and S of the 16^3 cells: 64-bit LDS counters of all cells (128 KiB), flushed once to the global ones
__global__ __launch_bounds__(PAL_WIDE_THREADS) void k_pal_bins(const i32x4 *__restrict__ points, long long n, long long stride,
                                                               unsigned long long *__restrict__ bins, long long share) {
  extern __shared__ unsigned long long pal_cnt[];           // [PAL_CELLS][4]
  for (int i = threadIdx.x; i < PAL_CELLS * 4; i += PAL_WIDE_THREADS) pal_cnt[i] = 0ull;
  __syncthreads();
  const int b = blockIdx.y;
  const long long p0 = (long long)blockIdx.x * share, p1 = p0 + share < n ? p0 + share : n;
  const i32x4 *pts = points + b * (stride / 2);
  for (long long p = p0 + 2LL * threadIdx.x; p < p1; p += 2LL * PAL_WIDE_THREADS) {
    const i32x4 v = pts[p >> 1];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (p + j >= p1) break;
      const PalPoint q = pal_unpack(v[2 * j], v[2 * j + 1]);
      if (q.w == 0u) continue;
      unsigned long long *c = pal_cnt + 4 * pal_cell(q);
      const long long w = (long long)q.w;
      atomicAdd(c, (unsigned long long)w);
      atomicAdd(c + 1, (unsigned long long)(w * q.L));
      atomicAdd(c + 2, (unsigned long long)(w * q.a));
      atomicAdd(c + 3, (unsigned long long)(w * q.b));
    }
  }
  __syncthreads();
  unsigned long long *out = bins + (size_t)b * PAL_CELLS * 4;
  for (int i = threadIdx.x; i < PAL_CELLS * 4; i += PAL_WIDE_THREADS) {
    const unsigned long long v = pal_cnt[i];
    if (v) atomicAdd(out + i, v);
  }
}

// weighted farthest-point selection over the cells, one workgroup per image: thread t owns cells 4 t .. 4 t + 3
__global__ __launch_bounds__(PAL_WIDE_THREADS) void k_pal_seeds(const long long *__restrict__ bins, int K, int *__restrict__ centres) {
  __shared__ PalBest best[PAL_WIDE_THREADS];
  __shared__ int seed[3];
  const int b = blockIdx.x, t = threadIdx.x;
  const long long *cells = bins + (size_t)b * PAL_CELLS * 4;
  unsigned long long W[PAL_CELLS_PER_THREAD], mind[PAL_CELLS_PER_THREAD];
  int m[PAL_CELLS_PER_THREAD][3];
#pragma unroll
  for (int j = 0; j < PAL_CELLS_PER_THREAD; ++j) {
    const long long *c = cells + 4 * (PAL_CELLS_PER_THREAD * t + j);
    const long long w = c[0];
    W[j] = (unsigned long long)w;
    mind[j] = 1ull;                                          // seed 0: the heaviest cell
#pragma unroll
    for (int a = 0; a < 3; ++a) m[j][a] = w > 0 ? pal_mean(c[1 + a], w) : 0;
  }
  int *out = centres + (size_t)b * K * 3;
  int first[3] = {0, 0, 0};
  for (int s = 0; s < K; ++s) {
    PalBest mine = {0ull, 0ull, PAL_CELLS};
#pragma unroll
    for (int j = 0; j < PAL_CELLS_PER_THREAD; ++j) {
      const U128 sc = mul128(W[j], mind[j]);
      const PalBest cand = {sc.hi, sc.lo, PAL_CELLS_PER_THREAD * t + j};
      if (pal_better(cand, mine)) mine = cand;
    }
    best[t] = mine;
    __syncthreads();
    for (int half = PAL_WIDE_THREADS / 2; half > 0; half >>= 1) {
      if (t < half && pal_better(best[t + half], best[t])) best[t] = best[t + half];
      __syncthreads();
    }
    const PalBest win = best[0];
    if (t == 0) {
      // a maximum of 0: no weight at all (seed 0 is the origin), or every cell sits on a seed (copies of seed 0)
      const bool none = win.hi == 0ull && win.lo == 0ull;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const long long *c = cells + 4 * (none ? 0 : win.cell);
        seed[a] = none ? first[a] : pal_mean(c[1 + a], c[0]);
        out[3 * s + a] = seed[a];
      }
    }
    __syncthreads();                                         // publishes seed; best[] is free again
    if (s == 0) {
#pragma unroll
      for (int a = 0; a < 3; ++a) first[a] = seed[a];
    }
#pragma unroll
    for (int j = 0; j < PAL_CELLS_PER_THREAD; ++j) {
      const unsigned long long d = pal_d2(m[j][0], m[j][1], m[j][2], seed[0], seed[1], seed[2]);
      mind[j] = s == 0 ? d : (d < mind[j] ? d : mind[j]);
    }
    __syncthreads();                                         // seed[] is read before thread 0 writes the next one
  }
}

// one Lloyd step: nearest centre of every weighted point of `assign`, W and S of `value` per cluster, optionally the labels
__global__ __launch_bounds__(PAL_THREADS) void k_pal_step(const i32x4 *__restrict__ assign, const i32x4 *__restrict__ value,
                                                          long long n, long long stride, const int *__restrict__ centres, int K,
                                                          unsigned long long *__restrict__ sums, uint8_t *__restrict__ labels,
                                                          long long share) {
  __shared__ unsigned long long acc[PAL_COPIES][PAL_MAX_K][4];
  __shared__ int cen[PAL_MAX_K][3];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < PAL_COPIES * PAL_MAX_K * 4; i += PAL_THREADS) (&acc[0][0][0])[i] = 0ull;
  if ((int)threadIdx.x < K * 3) (&cen[0][0])[threadIdx.x] = centres[(size_t)b * K * 3 + threadIdx.x];
  __syncthreads();
  const long long p0 = (long long)blockIdx.x * share, p1 = p0 + share < n ? p0 + share : n;
  const i32x4 *pa = assign + b * (stride / 2), *pv = value + b * (stride / 2);
  const bool paired = value != assign;
  const int copy = threadIdx.x & (PAL_COPIES - 1);
  for (long long p = p0 + 2LL * threadIdx.x; p < p1; p += 2LL * PAL_THREADS) {
    const i32x4 va = pa[p >> 1];
    i32x4 vv = va;
    if (paired) vv = pv[p >> 1];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (p + j >= p1) break;
      const PalPoint q = pal_unpack(va[2 * j], va[2 * j + 1]);
      int k = 255;
      if (q.w != 0u) {
        unsigned long long dmin = ~0ull;
        for (int c = 0; c < K; ++c) {
          const unsigned long long d = pal_d2(q.L, q.a, q.b, cen[c][0], cen[c][1], cen[c][2]);
          if (d < dmin) {                                    // strict: the lowest index wins a tie
            dmin = d;
            k = c;
          }
        }
        const PalPoint u = pal_unpack(vv[2 * j], vv[2 * j + 1]);
        const long long w = (long long)q.w;
        unsigned long long *a4 = acc[copy][k];
        atomicAdd(a4, (unsigned long long)w);
        atomicAdd(a4 + 1, (unsigned long long)(w * u.L));
        atomicAdd(a4 + 2, (unsigned long long)(w * u.a));
        atomicAdd(a4 + 3, (unsigned long long)(w * u.b));
      }
      if (labels) labels[(size_t)b * n + p + j] = (uint8_t)k;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < K * 4) {
    unsigned long long s = 0ull;
#pragma unroll
    for (int c = 0; c < PAL_COPIES; ++c) s += (&acc[c][0][0])[threadIdx.x];
    if (s) atomicAdd(sums + (size_t)b * K * 4 + threadIdx.x, s);
  }
}

// c_k = floor((2 S_k + W_k) / (2 W_k)); an empty cluster keeps its centre; optionally the sums are zeroed for the next step
__global__ __launch_bounds__(64) void k_pal_update(long long *__restrict__ sums, int K, int *__restrict__ centres, int clear) {
  const int b = blockIdx.x, t = threadIdx.x;
  long long *s = sums + (size_t)b * K * 4;
  long long W = 0, S = 0;
  if (t < K * 3) {
    W = s[4 * (t / 3)];
    S = s[4 * (t / 3) + 1 + t % 3];
  }
  __syncthreads();
  if (t < K * 3 && W > 0) centres[(size_t)b * K * 3 + t] = pal_mean(S, W);
  if (clear && t < K * 4) s[t] = 0;
}

// sigma of the transfer: the given one, or the mean distance over the live pairs of source centres (1 when there is none)
__global__ void k_pal_sigma(const float *__restrict__ src, const int *__restrict__ live, int K, float sigma,
                            float *__restrict__ sigma_used) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (sigma > 0.f) {
    *sigma_used = sigma;
    return;
  }
  double sum = 0.0;
  int pairs = 0;
  for (int i = 0; i < K; ++i) {
    if (!live[i]) continue;
    for (int j = i + 1; j < K; ++j) {
      if (!live[j]) continue;
      const double d0 = (double)src[3 * i] - (double)src[3 * j], d1 = (double)src[3 * i + 1] - (double)src[3 * j + 1],
                   d2 = (double)src[3 * i + 2] - (double)src[3 * j + 2];
      sum += sqrt(d0 * d0 + d1 * d1 + d2 * d2);
      ++pairs;
    }
  }
  const double mean = pairs ? sum / pairs : 0.0;
  *sigma_used = mean > 0.0 ? (float)mean : 1.f;
}

// y = x + sum_k u_k (t_k - s_k) / sum_k u_k in Lab, fp64, four pixels per lane; the output as k_idt_apply writes it
template <bool OU8>
__global__ __launch_bounds__(PAL_THREADS) void k_pal_transfer(const float *__restrict__ x, long long n, long long ps, long long cs,
                                                              const float *__restrict__ src, const float *__restrict__ dst,
                                                              const int *__restrict__ live, int K,
                                                              const float *__restrict__ sigma_used, void *__restrict__ ov) {
  __shared__ double s[PAL_MAX_K][3], shift[PAL_MAX_K][3];
  __shared__ int nlive;
  if (threadIdx.x == 0) {
    int m = 0;
    for (int k = 0; k < K; ++k) {
      if (!live[k]) continue;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        s[m][a] = (double)src[3 * k + a];
        shift[m][a] = (double)dst[3 * k + a] - (double)src[3 * k + a];
      }
      ++m;
    }
    nlive = m;
  }
  __syncthreads();
  const int M = nlive;
  const double sg = (double)*sigma_used, inv = 1.0 / (2.0 * sg * sg);
  const long long p = ((long long)blockIdx.x * PAL_THREADS + threadIdx.x) * 4;
  if (p >= n) return;
  float res[12];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float *px = x + (p + j < n ? p + j : n - 1) * ps;
    const double c[3] = {(double)hg_clamp01(px[0]), (double)hg_clamp01(px[cs]), (double)hg_clamp01(px[2 * cs])};
    double lab[3], unused0[3], unused1[3];
    hg_lab::srgb_to_lab_f64<false>(c, lab, unused0, unused1);
    double dmin = INFINITY;
    for (int k = 0; k < M; ++k) {
      const double d0 = lab[0] - s[k][0], d1 = lab[1] - s[k][1], d2 = lab[2] - s[k][2];
      dmin = fmin(dmin, d0 * d0 + d1 * d1 + d2 * d2);
    }
    double den = 0.0, num[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < M; ++k) {
      const double d0 = lab[0] - s[k][0], d1 = lab[1] - s[k][1], d2 = lab[2] - s[k][2];
      const double u = exp(-((d0 * d0 + d1 * d1 + d2 * d2) - dmin) * inv);
      den += u;
#pragma unroll
      for (int a = 0; a < 3; ++a) num[a] += u * shift[k][a];
    }
    if (M > 0) {
#pragma unroll
      for (int a = 0; a < 3; ++a) lab[a] += num[a] / den;
    }
    float rgb[3];
    hg_lab::lab_f64_to_srgb(lab, rgb);
#pragma unroll
    for (int a = 0; a < 3; ++a) res[3 * j + a] = rgb[a];
  }
  if constexpr (OU8) {
    uint8_t *o = static_cast<uint8_t *>(ov) + 3 * p;
    uint8_t q8[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) q8[i] = (uint8_t)(res[i] * 255.f);
    if (p + 3 < n) {
      *reinterpret_cast<HgBytes12 *>(o) = hg_pack_rgb4([&](int k) { return q8[k]; });
    } else {
      for (int i = 0; i < 3 * (int)(n - p); ++i) o[i] = q8[i];
    }
  } else {
    float *o = static_cast<float *>(ov) + 3 * p;
    if (p + 3 < n) {
#pragma unroll
      for (int w = 0; w < 3; ++w) {
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = res[4 * w + i];
        reinterpret_cast<f32x4 *>(o)[w] = v;
      }
    } else {
      for (int i = 0; i < 3 * (int)(n - p); ++i) o[i] = res[i];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
size_t pal_up16(size_t v) { return (v + 15) & ~(size_t)15; }

struct PalWorkspace {
  size_t points, other, bins, sums_other, total;
};

PalWorkspace pal_workspace(int B, long long n, bool paired) {
  PalWorkspace w;
  size_t o = 0;
  const size_t pts = pal_up16((size_t)B * pal_stride(n) * 8);
  w.points = o; o += pts;
  w.other = o; o += paired ? pts : 0;
  w.bins = o; o += (size_t)B * PAL_CELLS * 4 * sizeof(uint64_t);
  w.sums_other = o; o += paired ? pal_up16((size_t)B * PAL_MAX_K * 4 * sizeof(uint64_t)) : 0;
  w.total = o;
  return w;
}

int pal_check_k(int K) { return K < 1 || K > PAL_MAX_K ? HG_EPALETTE_K : HG_OK; }
int pal_check_pixels(long long n) { return n < 1 || n > PAL_MAX_PIXELS ? HG_EPALETTE_PIXELS : HG_OK; }
bool pal_batch_ok(int B) { return B >= 1 && B <= PAL_MAX_BATCH; }
bool pal_blocks_ok(int blocks) { return blocks >= 0 && blocks <= PAL_MAX_BLOCKS; }
bool pal_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int pal_quantize(const float *x, long long xs_b, long long xs_c, long long xs_h, long long xs_w, const float *wt, long long ws_b,
                 long long ws_h, long long ws_w, int16_t *points, int B, long long n, int W, hipStream_t st) {
  const long long stride = pal_stride(n), pairs = stride / 2;
  return launch(k_pal_quantize, dim3((unsigned)((pairs + PAL_THREADS - 1) / PAL_THREADS), B), dim3(PAL_THREADS), 0, st, x, xs_b, xs_c,
                xs_h, xs_w, wt, ws_b, ws_h, ws_w, reinterpret_cast<i32x4 *>(points), n, stride, W);
}

int pal_bins(const int16_t *points, int B, long long n, int64_t *bins, int blocks, hipStream_t st) {
  const PalShare s = pal_share(n, blocks);
  return launch(k_pal_bins, dim3(s.blocks, B), dim3(PAL_WIDE_THREADS), (size_t)PAL_CELLS * 4 * sizeof(unsigned long long), st,
                reinterpret_cast<const i32x4 *>(points), n, pal_stride(n), reinterpret_cast<unsigned long long *>(bins), s.share);
}

int pal_seeds(const int64_t *bins, int B, int K, int32_t *centres, hipStream_t st) {
  return launch(k_pal_seeds, dim3(B), dim3(PAL_WIDE_THREADS), 0, st, reinterpret_cast<const long long *>(bins), K, centres);
}

int pal_step(const int16_t *assign, const int16_t *value, int B, long long n, const int32_t *centres, int K, int64_t *sums,
             uint8_t *labels, int blocks, hipStream_t st) {
  const PalShare s = pal_share(n, blocks);
  return launch(k_pal_step, dim3(s.blocks, B), dim3(PAL_THREADS), 0, st, reinterpret_cast<const i32x4 *>(assign),
                reinterpret_cast<const i32x4 *>(value), n, pal_stride(n), centres, K, reinterpret_cast<unsigned long long *>(sums),
                labels, s.share);
}

int pal_update(int64_t *sums, int B, int K, int32_t *centres, int clear, hipStream_t st) {
  return launch(k_pal_update, dim3(B), dim3(64), 0, st, reinterpret_cast<long long *>(sums), K, centres, clear);
}

int pal_memset(void *p, size_t bytes, hipStream_t st) {
  const hipError_t e = hipMemsetAsync(p, 0, bytes, st);
  return e == hipSuccess ? HG_OK : (int)e;
}

}  // namespace

extern "C" {

int hg_palette_max_k(void) { return PAL_MAX_K; }
int hg_palette_blocks(int64_t n) { return pal_check_pixels(n) ? 0 : pal_plan_blocks(n); }
int64_t hg_palette_point_stride(int64_t n) { return pal_check_pixels(n) ? 0 : pal_stride(n); }

size_t hg_palette_workspace_bytes(int32_t B, int64_t n, int32_t paired) {
  if (!pal_batch_ok(B) || pal_check_pixels(n)) return 0;
  return pal_workspace(B, n, paired != 0).total;
}

int hg_palette_quantize(const float *x, int64_t xs_b, int64_t xs_c, int64_t xs_h, int64_t xs_w, const float *weight, int64_t ws_b,
                        int64_t ws_h, int64_t ws_w, int16_t *points, int32_t B, int32_t H, int32_t W, void *stream) {
  if (!x || !points || !pal_aligned16(points) || !pal_batch_ok(B) || H < 1 || W < 1) return HG_EINVAL;
  if (int rc = pal_check_pixels((long long)H * W)) return rc;
  return pal_quantize(x, xs_b, xs_c, xs_h, xs_w, weight, ws_b, ws_h, ws_w, points, B, (long long)H * W, W, (hipStream_t)stream);
}

int hg_palette_bins(const int16_t *points, int32_t B, int64_t n, int64_t *bins, int32_t blocks, void *stream) {
  if (!points || !bins || !pal_aligned16(points) || !pal_batch_ok(B) || !pal_blocks_ok(blocks)) return HG_EINVAL;
  if (int rc = pal_check_pixels(n)) return rc;
  return pal_bins(points, B, n, bins, blocks, (hipStream_t)stream);
}

int hg_palette_seeds(const int64_t *bins, int32_t B, int32_t K, int32_t *centres, void *stream) {
  if (!bins || !centres || !pal_batch_ok(B)) return HG_EINVAL;
  if (int rc = pal_check_k(K)) return rc;
  return pal_seeds(bins, B, K, centres, (hipStream_t)stream);
}

int hg_palette_step(const int16_t *assign, const int16_t *value, int32_t B, int64_t n, const int32_t *centres, int32_t K,
                    int64_t *sums, uint8_t *labels, int32_t blocks, void *stream) {
  if (!assign || !value || !centres || !sums || !pal_aligned16(assign) || !pal_aligned16(value) || !pal_batch_ok(B) ||
      !pal_blocks_ok(blocks))
    return HG_EINVAL;
  if (int rc = pal_check_k(K)) return rc;
  if (int rc = pal_check_pixels(n)) return rc;
  return pal_step(assign, value, B, n, centres, K, sums, labels, blocks, (hipStream_t)stream);
}

int hg_palette_update(int64_t *sums, int32_t B, int32_t K, int32_t *centres, int32_t clear_sums, void *stream) {
  if (!sums || !centres || !pal_batch_ok(B)) return HG_EINVAL;
  if (int rc = pal_check_k(K)) return rc;
  return pal_update(sums, B, K, centres, clear_sums != 0, (hipStream_t)stream);
}

int hg_palette_run(const float *x, int64_t xs_b, int64_t xs_c, int64_t xs_h, int64_t xs_w, const float *weight, int64_t ws_b,
                   int64_t ws_h, int64_t ws_w, const float *other, int64_t os_b, int64_t os_c, int64_t os_h, int64_t os_w,
                   int32_t B, int32_t H, int32_t W, int32_t K, int32_t iterations, int32_t blocks, int32_t *centres,
                   int64_t *sums, int32_t *centres_other, uint8_t *labels, void *workspace, size_t workspace_bytes,
                   void *stream) {
  if (!x || !centres || !sums || !workspace || !pal_aligned16(workspace) || !pal_batch_ok(B) || H < 1 || W < 1 ||
      iterations < 0 || !pal_blocks_ok(blocks) || (other != nullptr) != (centres_other != nullptr))
    return HG_EINVAL;
  if (int rc = pal_check_k(K)) return rc;
  const long long n = (long long)H * W;
  if (int rc = pal_check_pixels(n)) return rc;
  const PalWorkspace w = pal_workspace(B, n, other != nullptr);
  if (workspace_bytes < w.total) return HG_EWORKSPACE;
  char *base = static_cast<char *>(workspace);
  int16_t *pts = reinterpret_cast<int16_t *>(base + w.points), *pts_other = reinterpret_cast<int16_t *>(base + w.other);
  int64_t *bins = reinterpret_cast<int64_t *>(base + w.bins), *sums_other = reinterpret_cast<int64_t *>(base + w.sums_other);
  hipStream_t st = (hipStream_t)stream;
  const size_t sum_bytes = (size_t)B * K * 4 * sizeof(int64_t), centre_bytes = (size_t)B * K * 3 * sizeof(int32_t);
  int rc = pal_memset(bins, (size_t)B * PAL_CELLS * 4 * sizeof(int64_t), st);
  if (!rc) rc = pal_memset(sums, sum_bytes, st);
  if (!rc) rc = pal_quantize(x, xs_b, xs_c, xs_h, xs_w, weight, ws_b, ws_h, ws_w, pts, B, n, W, st);
  if (!rc) rc = pal_bins(pts, B, n, bins, blocks, st);
  if (!rc) rc = pal_seeds(bins, B, K, centres, st);
  for (int i = 0; i < iterations && !rc; ++i) {
    rc = pal_step(pts, pts, B, n, centres, K, sums, nullptr, blocks, st);
    if (!rc) rc = pal_update(sums, B, K, centres, 1, st);
  }
  if (!rc) rc = pal_step(pts, pts, B, n, centres, K, sums, labels, blocks, st);
  if (other && !rc) {
    // the paired palette: the means of `other` and of the image over each cluster's pixels; an empty cluster keeps the centre
    rc = pal_quantize(other, os_b, os_c, os_h, os_w, nullptr, 0, 0, 0, pts_other, B, n, W, st);
    if (!rc) rc = pal_memset(sums_other, sum_bytes, st);
    if (!rc) {
      const hipError_t e = hipMemcpyAsync(centres_other, centres, centre_bytes, hipMemcpyDeviceToDevice, st);
      rc = e == hipSuccess ? HG_OK : (int)e;
    }
    if (!rc) rc = pal_step(pts, pts_other, B, n, centres, K, sums_other, nullptr, blocks, st);
    if (!rc) rc = pal_update(sums_other, B, K, centres_other, 0, st);
    if (!rc) rc = pal_update(sums, B, K, centres, 0, st);      // both palettes are means over the clusters of the last step
  }
  return rc;
}

int hg_palette_transfer(const float *x, int64_t n, int64_t pix_stride, int64_t chan_stride, const float *src_centres,
                        const float *dst_centres, const int32_t *live, int32_t K, float sigma, float *sigma_used, void *out,
                        int32_t out_u8, void *stream) {
  if (!x || !src_centres || !dst_centres || !live || !sigma_used || !out || pix_stride <= 0 || chan_stride <= 0 ||
      (reinterpret_cast<uintptr_t>(out) & (out_u8 ? 3 : 15)) || sigma != sigma || sigma == INFINITY)
    return HG_EINVAL;
  if (int rc = pal_check_k(K)) return rc;
  if (int rc = pal_check_pixels(n)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch(k_pal_sigma, dim3(1), dim3(64), 0, st, src_centres, live, K, sigma, sigma_used)) return rc;
  const long long groups = (n + 3) / 4;
  const dim3 grid((unsigned)((groups + PAL_THREADS - 1) / PAL_THREADS));
  return dispatch([&](auto OU8) {
    return launch(k_pal_transfer<OU8>, grid, dim3(PAL_THREADS), 0, st, x, n, pix_stride, chan_stride, src_centres, dst_centres, live, K,
                  sigma_used, out);
  }, out_u8 != 0);
}

}  // extern "C"
