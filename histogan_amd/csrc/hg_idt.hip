// hg_idt.hip -- iterative distribution transfer (include/hg_post.h, hg_idt_*): the nonlinear colour transfer of Pitie et
// al.  Per rotation the colour cloud is projected on three orthogonal axes and each 1-D marginal is matched to the
// target's by CDF matching.  Everything that decides the map is an integer: pixels deposit 65536 units each into
// linear-binned histograms through LDS integer atomics, workgroups add their counters to 64-bit global counters, and the
// quantile search compares 128-bit products -- so the result does not depend on the order of any sum and repeats are
// bit-identical.  The per-pixel passes are streaming work bound by HBM bandwidth: the working copy of the source is three
// planes, four pixels (16 bytes per plane) per lane.
#include "hg_host.h"
#include "../../include/hg_post.h"

namespace {

constexpr int IDT_THREADS = 256;
constexpr int IDT_BLOCK_PIXELS = 65532;      // per pass over the LDS counters: < 65536 (65536 units each fit a uint32), % 4 == 0
constexpr int IDT_MAX_BINS = 4096;
constexpr int IDT_LDS_COUNTERS = 3 * IDT_MAX_BINS;          // 48 KiB of uint32 counters / of fp32 map nodes
constexpr int IDT_SHARE_PIXELS = 4096;       // the plan gives a workgroup at least this many pixels ...
constexpr int IDT_MAX_BLOCKS = 2048;         // ... and a launch at most this many workgroups
constexpr long long IDT_MAX_PIXELS = 0xffffffffLL;
constexpr uint32_t IDT_RANGE_LO_INIT = 0xffffffffu, IDT_RANGE_HI_INIT = 0u;
static_assert(IDT_BLOCK_PIXELS % 4 == 0 && IDT_BLOCK_PIXELS <= 65535, "a uint32 counter holds 65535 pixels of 65536 units");

// order-preserving unsigned image of a float: integer atomicMin / atomicMax then order as the floats do
__host__ __device__ inline uint32_t idt_enc(float f) {
  union { float f; uint32_t u; } c;
  c.f = f;
  return (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
}

__host__ __device__ inline float idt_dec(uint32_t e) {
  union { float f; uint32_t u; } c;
  c.u = (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e;
  return c.f;
}

struct IdtRot {
  float r[9];       // row a = axis a
};

__device__ __forceinline__ IdtRot idt_load_rot(const float *__restrict__ rot) {
  IdtRot R;
#pragma unroll
  for (int i = 0; i < 9; ++i) R.r[i] = rot[i];
  return R;
}

// one fixed evaluation order in every kernel: the minimum a range pass finds is the value the histogram pass bins
__device__ __forceinline__ float idt_project(const IdtRot &R, int a, float x0, float x1, float x2) {
  return fmaf(R.r[3 * a + 2], x2, fmaf(R.r[3 * a + 1], x1, R.r[3 * a] * x0));
}

struct IdtAxis {
  float lo, den;    // den = hi - lo
  bool live;        // hi - lo > 2^-20
};

__device__ __forceinline__ IdtAxis idt_axis(const uint32_t *__restrict__ range, int a) {
  IdtAxis ax;
  ax.lo = idt_dec(range[a]);
  ax.den = idt_dec(range[3 + a]) - ax.lo;
  ax.live = ax.den > 0x1p-20f;
  return ax;
}

// node and fraction of a projected value (step 2); every pixel of a degenerate axis sits on node 0
__device__ __forceinline__ void idt_bin(float v, const IdtAxis &ax, int bins, int &k, float &t) {
  const float nm1 = (float)(bins - 1);
  float u = ax.live ? (v - ax.lo) * nm1 / ax.den : 0.f;
  u = fminf(fmaxf(u, 0.f), nm1);               // a NaN becomes 0
  k = min((int)u, bins - 2);
  t = u - (float)k;
}

struct IdtShare {
  int blocks;
  long long share;  // pixels of a workgroup, % 4 == 0
};

int idt_plan_blocks(long long n) {
  const long long b = (n + IDT_SHARE_PIXELS - 1) / IDT_SHARE_PIXELS;
  return (int)(b < 1 ? 1 : (b > IDT_MAX_BLOCKS ? IDT_MAX_BLOCKS : b));
}

IdtShare idt_share(long long n, int blocks) {
  IdtShare s;
  s.blocks = blocks > 0 ? blocks : idt_plan_blocks(n);
  s.share = ((n + s.blocks - 1) / s.blocks + 3) & ~3LL;
  return s;
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IDT_THREADS) void k_idt_clear(uint32_t *__restrict__ ranges, long long n_sets,
                                                           unsigned long long *__restrict__ hist, long long n_counters) {
  const long long i0 = (long long)blockIdx.x * IDT_THREADS + threadIdx.x, step = (long long)gridDim.x * IDT_THREADS;
  for (long long i = i0; i < n_sets * 6; i += step) ranges[i] = (i % 6) < 3 ? IDT_RANGE_LO_INIT : IDT_RANGE_HI_INIT;
  for (long long i = i0; i < n_counters; i += step) hist[i] = 0ull;
}

// block-wide min / max of the three axes, then six global integer atomics
__device__ __forceinline__ void idt_range_commit(float (&mn)[3], float (&mx)[3], float (*sm)[6], uint32_t *__restrict__ range) {
  const int wv = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn[a] = fminf(mn[a], __shfl_xor(mn[a], o, 64));
      mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
      sm[wv][a] = mn[a];
      sm[wv][3 + a] = mx[a];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int t = threadIdx.x;
    if (t < 3) {
      const float v = fminf(fminf(sm[0][t], sm[1][t]), fminf(sm[2][t], sm[3][t]));
      if (v < INFINITY) atomicMin(range + t, idt_enc(v));
    } else {
      const float v = fmaxf(fmaxf(sm[0][t], sm[1][t]), fmaxf(sm[2][t], sm[3][t]));
      if (v > -INFINITY) atomicMax(range + t, idt_enc(v));
    }
  }
  __syncthreads();
}

// min / max of the projections of n strided pixels for nrot rotations; optionally the planar working copy
__global__ __launch_bounds__(IDT_THREADS) void k_idt_range(const float *__restrict__ x, long long n, long long ps,
                                                           long long cs, const float *__restrict__ rot, int nrot,
                                                           uint32_t *__restrict__ ranges, float *__restrict__ planes,
                                                           long long np, long long share) {
  __shared__ float sm[4][6];
  const long long p0 = (long long)blockIdx.x * share, p1 = p0 + share < n ? p0 + share : n;
  for (int r = 0; r < nrot; ++r) {
    const IdtRot R = idt_load_rot(rot + 9 * r);
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long p = p0 + threadIdx.x; p < p1; p += IDT_THREADS) {
      const float *px = x + p * ps;
      const float x0 = px[0], x1 = px[cs], x2 = px[2 * cs];
      if (planes && r == 0) {
        planes[p] = x0; planes[np + p] = x1; planes[2 * np + p] = x2;
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float v = idt_project(R, a, x0, x1, x2);
        mn[a] = fminf(mn[a], v);
        mx[a] = fmaxf(mx[a], v);
      }
    }
    idt_range_commit(mn, mx, sm, ranges + 6 * r);
  }
}

// linear-binned fixed-point histograms of nrot rotations: LDS uint32 counters, flushed to the global uint64 counters
// after every IDT_BLOCK_PIXELS pixels.  VEC = 4: the planar working copy (ps == 1), 16 bytes per lane and plane.
template <int VEC>
__global__ __launch_bounds__(IDT_THREADS) void k_idt_hist(const float *__restrict__ x, long long n, long long ps,
                                                          long long cs, const float *__restrict__ rot, int nrot, int bins,
                                                          const uint32_t *__restrict__ ranges,
                                                          unsigned long long *__restrict__ hist, long long share) {
  extern __shared__ uint32_t idt_cnt[];
  const int used = nrot * 3 * bins;
  const long long b0 = (long long)blockIdx.x * share, b1 = b0 + share < n ? b0 + share : n;
  for (long long q0 = b0; q0 < b1; q0 += IDT_BLOCK_PIXELS) {
    const long long q1 = q0 + IDT_BLOCK_PIXELS < b1 ? q0 + IDT_BLOCK_PIXELS : b1;
    for (int i = threadIdx.x; i < used; i += IDT_THREADS) idt_cnt[i] = 0u;
    __syncthreads();
    for (int r = 0; r < nrot; ++r) {
      const IdtRot R = idt_load_rot(rot + 9 * r);
      IdtAxis ax[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) ax[a] = idt_axis(ranges + 6 * r, a);
      uint32_t *cr = idt_cnt + r * 3 * bins;
      for (long long p = q0 + (long long)threadIdx.x * VEC; p < q1; p += (long long)IDT_THREADS * VEC) {
        float c[3][VEC];
        if constexpr (VEC == 4) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(x + ch * cs + p);
#pragma unroll
            for (int j = 0; j < 4; ++j) c[ch][j] = v[j];
          }
        } else {
          const float *px = x + p * ps;
          c[0][0] = px[0]; c[1][0] = px[cs]; c[2][0] = px[2 * cs];
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          if (p + j >= q1) break;
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            int k;
            float t;
            idt_bin(idt_project(R, a, c[0][j], c[1][j], c[2][j]), ax[a], bins, k, t);
            const uint32_t q = (uint32_t)floorf(t * 65536.f + 0.5f);
            if (q != 65536u) atomicAdd(cr + a * bins + k, 65536u - q);
            if (q != 0u) atomicAdd(cr + a * bins + k + 1, q);
          }
        }
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < used; i += IDT_THREADS) {
      const uint32_t v = idt_cnt[i];
      if (v) atomicAdd(hist + i, (unsigned long long)v);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// exact products of two 64-bit integers
struct U128 {
  unsigned long long hi, lo;
};

__device__ __forceinline__ U128 mul128(unsigned long long a, unsigned long long b) { return {__umul64hi(a, b), a * b}; }
__device__ __forceinline__ bool ge128(const U128 &a, const U128 &b) { return a.hi != b.hi ? a.hi > b.hi : a.lo >= b.lo; }
__device__ __forceinline__ U128 sub128(const U128 &a, const U128 &b) {
  return {a.hi - b.hi - (a.lo < b.lo ? 1ull : 0ull), a.lo - b.lo};
}
__device__ __forceinline__ double dbl128(const U128 &a) { return (double)a.hi * 18446744073709551616.0 + (double)a.lo; }

// inclusive prefix sums of h[0..bins): thread t owns the run [t * run, (t + 1) * run).  Returns the sum in front of the
// thread's run and the total.
__device__ __forceinline__ void idt_run_offsets(const unsigned long long *__restrict__ h, int bins, int run,
                                                unsigned long long *sm_runs, unsigned long long &before,
                                                unsigned long long &total) {
  const int k0 = threadIdx.x * run, k1 = min(bins, k0 + run);
  unsigned long long s = 0ull;
  for (int k = k0; k < k1; ++k) s += h[k];
  sm_runs[threadIdx.x] = s;
  __syncthreads();
  before = 0ull;
  total = 0ull;
  for (int j = 0; j < IDT_THREADS; ++j) {
    const unsigned long long v = sm_runs[j];
    before += j < (int)threadIdx.x ? v : 0ull;
    total += v;
  }
}

// step 3, one workgroup per axis (grid = 3); then the axis' counters and the next rotation's range slots are reset
__global__ __launch_bounds__(IDT_THREADS) void k_idt_table(unsigned long long *__restrict__ src_hist,
                                                           const unsigned long long *__restrict__ tgt_hist,
                                                           const uint32_t *__restrict__ tgt_range, int bins,
                                                           float *__restrict__ map, uint32_t *__restrict__ next_range,
                                                           int clear_src) {
  __shared__ unsigned long long c1[IDT_MAX_BINS];
  __shared__ unsigned long long runs[2][IDT_THREADS];
  const int run = (bins + IDT_THREADS - 1) / IDT_THREADS, k0 = threadIdx.x * run, k1 = min(bins, k0 + run);
  const int a = blockIdx.x;
  const unsigned long long *h1 = tgt_hist + (size_t)a * bins;
  unsigned long long *h0 = src_hist + (size_t)a * bins;
  unsigned long long before1, T1, before0, T0;
  idt_run_offsets(h1, bins, run, runs[0], before1, T1);
  for (int k = k0; k < k1; ++k) {
    before1 += h1[k];
    c1[k] = before1;
  }
  idt_run_offsets(h0, bins, run, runs[1], before0, T0);        // (its barrier also publishes c1)
  const double lo1 = (double)idt_dec(tgt_range[a]), hi1 = (double)idt_dec(tgt_range[3 + a]);
  for (int k = k0; k < k1; ++k) {
    before0 += h0[k];
    const U128 lhs = mul128(before0, T1);
    int jl = 0, jh = bins - 1;                                 // smallest j with c1[j] T0 >= c0[k] T1
    while (jl < jh) {
      const int jm = (jl + jh) >> 1;
      if (ge128(mul128(c1[jm], T0), lhs)) jh = jm;
      else jl = jm + 1;
    }
    double up = 0.0;
    if (jl > 0) {
      const U128 below = mul128(c1[jl - 1], T0);
      const double den = dbl128(mul128(c1[jl] - c1[jl - 1], T0));
      up = (double)(jl - 1) + (den > 0.0 && ge128(lhs, below) ? dbl128(sub128(lhs, below)) / den : 0.0);
    }
    map[(size_t)a * bins + k] = (float)(lo1 + up / (double)(bins - 1) * (hi1 - lo1));
    if (clear_src) h0[k] = 0ull;
  }
  if (next_range && a == 0 && threadIdx.x < 6) next_range[threadIdx.x] = threadIdx.x < 3 ? IDT_RANGE_LO_INIT : IDT_RANGE_HI_INIT;
}

// ---------------------------------------------------------------------------------------------------------------------
// steps 4 and 5 and x += rho R^T d on the planar working copy, four pixels per lane.  LAST: clip and write the HWC output;
// otherwise write the copy back and reduce the range of the next rotation's projections in the same pass.
template <bool LAST, bool OU8>
__global__ __launch_bounds__(IDT_THREADS) void k_idt_apply(float *__restrict__ planes, long long n, long long np,
                                                           const float *__restrict__ rot, const float *__restrict__ rot_next,
                                                           int bins, const uint32_t *__restrict__ range,
                                                           const float *__restrict__ map, float rho,
                                                           uint32_t *__restrict__ next_range, void *__restrict__ ov,
                                                           long long share) {
  extern __shared__ float idt_map[];
  __shared__ float sm[4][6];
  for (int i = threadIdx.x; i < 3 * bins; i += IDT_THREADS) idt_map[i] = map[i];
  const IdtRot R = idt_load_rot(rot);
  IdtRot Rn = R;
  if constexpr (!LAST) Rn = idt_load_rot(rot_next);
  IdtAxis ax[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) ax[a] = idt_axis(range, a);
  __syncthreads();
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  const long long b0 = (long long)blockIdx.x * share, b1 = b0 + share < n ? b0 + share : n;
  for (long long p = b0 + (long long)threadIdx.x * 4; p < b1; p += (long long)IDT_THREADS * 4) {
    f32x4 c[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch] = *reinterpret_cast<const f32x4 *>(planes + ch * np + p);
    float res[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float x0 = c[0][j], x1 = c[1][j], x2 = c[2][j], d[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float v = idt_project(R, a, x0, x1, x2);
        int k;
        float t;
        idt_bin(v, ax[a], bins, k, t);
        const float *m = idt_map + a * bins + k;
        const float vn = fmaf(t, m[1], (1.f - t) * m[0]);
        d[a] = ax[a].live ? vn - v : 0.f;
      }
      x0 = fmaf(rho, fmaf(R.r[6], d[2], fmaf(R.r[3], d[1], R.r[0] * d[0])), x0);      // explicit fma's: the middle and the last
      x1 = fmaf(rho, fmaf(R.r[7], d[2], fmaf(R.r[4], d[1], R.r[1] * d[0])), x1);      // rotation's instantiations round alike
      x2 = fmaf(rho, fmaf(R.r[8], d[2], fmaf(R.r[5], d[1], R.r[2] * d[0])), x2);
      if constexpr (LAST) {
        res[3 * j] = hg_clamp01(x0);
        res[3 * j + 1] = hg_clamp01(x1);
        res[3 * j + 2] = hg_clamp01(x2);
      } else {
        c[0][j] = x0; c[1][j] = x1; c[2][j] = x2;
        if (p + j < b1) {
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            const float v = idt_project(Rn, a, x0, x1, x2);
            mn[a] = fminf(mn[a], v);
            mx[a] = fmaxf(mx[a], v);
          }
        }
      }
    }
    if constexpr (!LAST) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) *reinterpret_cast<f32x4 *>(planes + ch * np + p) = c[ch];     // p + 3 < np
    } else if constexpr (OU8) {
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
  if constexpr (!LAST) idt_range_commit(mn, mx, sm, next_range);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
long long idt_plane_stride(long long n) { return (n + 3) & ~3LL; }

size_t idt_up16(size_t v) { return (v + 15) & ~(size_t)15; }

struct IdtWorkspace {
  size_t planes, map, src_range, tgt_range, src_hist, tgt_hist, total;
};

IdtWorkspace idt_workspace(long long n_src, int iterations, int bins) {
  IdtWorkspace w;
  size_t o = 0;
  w.planes = o; o += idt_up16((size_t)3 * idt_plane_stride(n_src) * sizeof(float));
  w.map = o; o += idt_up16((size_t)3 * bins * sizeof(float));
  w.src_range = o; o += idt_up16(2 * 6 * sizeof(uint32_t));
  w.tgt_range = o; o += idt_up16((size_t)iterations * 6 * sizeof(uint32_t));
  w.src_hist = o; o += idt_up16((size_t)3 * bins * sizeof(uint64_t));
  w.tgt_hist = o; o += idt_up16((size_t)iterations * 3 * bins * sizeof(uint64_t));
  w.total = o;
  return w;
}

int idt_check_bins(int bins) { return bins < 2 ? HG_EIDT_BINS : (bins > IDT_MAX_BINS ? HG_EIDT_BINS_LDS : HG_OK); }
int idt_check_pixels(long long n) { return n < 1 || n > IDT_MAX_PIXELS ? HG_EIDT_PIXELS : HG_OK; }
int idt_chunk(int bins) { return IDT_LDS_COUNTERS / (3 * bins); }

int idt_clear(uint32_t *ranges, long long n_sets, uint64_t *hist, long long n_counters, hipStream_t st) {
  const long long items = n_sets * 6 > n_counters ? n_sets * 6 : n_counters;
  long long nb = (items + IDT_THREADS - 1) / IDT_THREADS;
  nb = nb < 1 ? 1 : (nb > IDT_MAX_BLOCKS ? IDT_MAX_BLOCKS : nb);
  return launch(k_idt_clear, dim3((unsigned)nb), dim3(IDT_THREADS), 0, st, ranges, n_sets,
                reinterpret_cast<unsigned long long *>(hist), n_counters);
}

int idt_range(const float *x, long long n, long long ps, long long cs, const float *rot, int nrot, uint32_t *ranges,
              float *planes, hipStream_t st) {
  const IdtShare s = idt_share(n, 0);
  return launch(k_idt_range, dim3(s.blocks), dim3(IDT_THREADS), 0, st, x, n, ps, cs, rot, nrot, ranges, planes, idt_plane_stride(n),
                s.share);
}

int idt_hist(const float *x, long long n, long long ps, long long cs, const float *rot, int nrot, int bins,
             const uint32_t *ranges, uint64_t *hist, int blocks, hipStream_t st) {
  const IdtShare s = idt_share(n, blocks);
  const size_t lds = (size_t)nrot * 3 * bins * sizeof(uint32_t);
  unsigned long long *h = reinterpret_cast<unsigned long long *>(hist);
  const bool planar = ps == 1 && cs % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && cs >= idt_plane_stride(n);
  return dispatch([&](auto PLANAR) {
    return launch(k_idt_hist<PLANAR ? 4 : 1>, dim3(s.blocks), dim3(IDT_THREADS), lds, st, x, n, ps, cs, rot, nrot, bins, ranges, h,
                  s.share);
  }, planar);
}

int idt_table(uint64_t *src_hist, const uint64_t *tgt_hist, const uint32_t *tgt_range, int bins, float *map,
              uint32_t *next_range, int clear_src, hipStream_t st) {
  return launch(k_idt_table, dim3(3), dim3(IDT_THREADS), 0, st, reinterpret_cast<unsigned long long *>(src_hist),
                reinterpret_cast<const unsigned long long *>(tgt_hist), tgt_range, bins, map, next_range, clear_src);
}

int idt_apply(float *planes, long long n, const float *rot, const float *rot_next, int bins, const uint32_t *range,
              const float *map, float rho, uint32_t *next_range, void *out, int out_u8, hipStream_t st) {
  const IdtShare s = idt_share(n, 0);
  const size_t lds = (size_t)3 * bins * sizeof(float);
  const long long np = idt_plane_stride(n);
  // the three instantiations there are: a middle rotation, the last one to fp32, the last one to uint8
  return dispatch([&](auto END) {
    return launch(k_idt_apply<END != 0, END == 2>, dim3(s.blocks), dim3(IDT_THREADS), lds, st, planes, n, np, rot, rot_next, bins,
                  range, map, rho, next_range, out, s.share);
  }, among<0, 1, 2>(rot_next ? 0 : (out_u8 ? 2 : 1)));
}

int idt_target_tables(const float *tgt, long long n, long long ps, long long cs, const float *rot, int iterations, int bins,
                      uint32_t *tgt_range, uint64_t *tgt_hist, hipStream_t st) {
  int rc = idt_range(tgt, n, ps, cs, rot, iterations, tgt_range, nullptr, st);
  const int chunk = idt_chunk(bins);
  for (int r = 0; r < iterations && !rc; r += chunk) {
    const int nr = iterations - r < chunk ? iterations - r : chunk;
    rc = idt_hist(tgt, n, ps, cs, rot + 9 * r, nr, bins, tgt_range + 6 * r, tgt_hist + (size_t)r * 3 * bins, 0, st);
  }
  return rc;
}

bool idt_strides_ok(int64_t ps, int64_t cs) { return ps > 0 && cs > 0; }

}  // namespace

extern "C" {

int hg_idt_block_pixels(void) { return IDT_BLOCK_PIXELS; }
int hg_idt_max_bins(void) { return IDT_MAX_BINS; }
int hg_idt_group_pixels(void) { return IDT_THREADS * 4; }
int hg_idt_target_chunk(int32_t bins) { return idt_check_bins(bins) ? 0 : idt_chunk(bins); }
int hg_idt_blocks(int64_t n) { return idt_check_pixels(n) ? 0 : idt_plan_blocks(n); }
int64_t hg_idt_plane_stride(int64_t n) { return idt_check_pixels(n) ? 0 : idt_plane_stride(n); }

size_t hg_idt_workspace_bytes(int64_t n_src, int64_t n_tgt, int32_t iterations, int32_t bins) {
  if (idt_check_pixels(n_src) || idt_check_pixels(n_tgt) || iterations < 1 || idt_check_bins(bins)) return 0;
  return idt_workspace(n_src, iterations, bins).total;
}

int hg_idt_clear(uint32_t *ranges, int64_t n_ranges, uint64_t *hist, int64_t n_counters, void *stream) {
  if (n_ranges < 0 || n_counters < 0 || (n_ranges > 0 && !ranges) || (n_counters > 0 && !hist)) return HG_EINVAL;
  if (n_ranges == 0 && n_counters == 0) return HG_OK;
  return idt_clear(ranges, n_ranges, hist, n_counters, (hipStream_t)stream);
}

int hg_idt_range(const float *x, int64_t n, int64_t pix_stride, int64_t chan_stride, const float *rotations, int32_t nrot,
                 uint32_t *ranges, float *planes, void *stream) {
  if (!x || !rotations || !ranges || !idt_strides_ok(pix_stride, chan_stride)) return HG_EINVAL;
  if (planes && (reinterpret_cast<uintptr_t>(planes) & 15)) return HG_EINVAL;
  if (nrot < 1) return HG_EIDT_ITERATIONS;
  if (int rc = idt_check_pixels(n)) return rc;
  return idt_range(x, n, pix_stride, chan_stride, rotations, nrot, ranges, planes, (hipStream_t)stream);
}

int hg_idt_hist(const float *x, int64_t n, int64_t pix_stride, int64_t chan_stride, const float *rotations, int32_t nrot,
                int32_t bins, const uint32_t *ranges, uint64_t *hist, int32_t blocks, void *stream) {
  if (!x || !rotations || !ranges || !hist || !idt_strides_ok(pix_stride, chan_stride) || blocks < 0 ||
      blocks > IDT_MAX_BLOCKS)
    return HG_EINVAL;
  if (int rc = idt_check_bins(bins)) return rc;
  if (nrot < 1 || nrot > idt_chunk(bins)) return HG_EIDT_ITERATIONS;
  if (int rc = idt_check_pixels(n)) return rc;
  return idt_hist(x, n, pix_stride, chan_stride, rotations, nrot, bins, ranges, hist, blocks, (hipStream_t)stream);
}

int hg_idt_table(uint64_t *src_hist, const uint64_t *tgt_hist, const uint32_t *tgt_range, int32_t bins, float *map,
                 uint32_t *next_range, int32_t clear_src_hist, void *stream) {
  if (!src_hist || !tgt_hist || !tgt_range || !map) return HG_EINVAL;
  if (int rc = idt_check_bins(bins)) return rc;
  return idt_table(src_hist, tgt_hist, tgt_range, bins, map, next_range, clear_src_hist != 0, (hipStream_t)stream);
}

int hg_idt_apply(float *planes, int64_t n, const float *rotation, const float *rotation_next, int32_t bins,
                 const uint32_t *range, const float *map, float relaxation, uint32_t *next_range, void *out, int32_t out_u8,
                 void *stream) {
  if (!planes || !rotation || !range || !map || (reinterpret_cast<uintptr_t>(planes) & 15)) return HG_EINVAL;
  if (rotation_next ? !next_range : (!out || (reinterpret_cast<uintptr_t>(out) & (out_u8 ? 3 : 15)))) return HG_EINVAL;
  if (int rc = idt_check_bins(bins)) return rc;
  if (!(relaxation > 0.f && relaxation <= 1.f)) return HG_EIDT_RELAXATION;
  if (int rc = idt_check_pixels(n)) return rc;
  return idt_apply(planes, n, rotation, rotation_next, bins, range, map, relaxation, next_range, out, out_u8,
                   (hipStream_t)stream);
}

int hg_idt_target_tables(const float *target, int64_t n, int64_t pix_stride, int64_t chan_stride, const float *rotations,
                         int32_t iterations, int32_t bins, uint32_t *tgt_range, uint64_t *tgt_hist, void *stream) {
  if (!target || !rotations || !tgt_range || !tgt_hist || !idt_strides_ok(pix_stride, chan_stride)) return HG_EINVAL;
  if (int rc = idt_check_bins(bins)) return rc;
  if (iterations < 1) return HG_EIDT_ITERATIONS;
  if (int rc = idt_check_pixels(n)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = idt_clear(tgt_range, iterations, tgt_hist, (long long)iterations * 3 * bins, st)) return rc;
  return idt_target_tables(target, n, pix_stride, chan_stride, rotations, iterations, bins, tgt_range, tgt_hist, st);
}

int hg_idt_run(const float *source, int64_t n_src, int64_t src_pix_stride, int64_t src_chan_stride, const float *target,
               int64_t n_tgt, int64_t tgt_pix_stride, int64_t tgt_chan_stride, const float *rotations, int32_t iterations,
               int32_t bins, float relaxation, void *out, int32_t out_u8, void *workspace, size_t workspace_bytes,
               void *stream) {
  if (!source || !target || !rotations || !out || !workspace || !idt_strides_ok(src_pix_stride, src_chan_stride) ||
      !idt_strides_ok(tgt_pix_stride, tgt_chan_stride) || (reinterpret_cast<uintptr_t>(workspace) & 15) ||
      (reinterpret_cast<uintptr_t>(out) & (out_u8 ? 3 : 15)))
    return HG_EINVAL;
  if (int rc = idt_check_bins(bins)) return rc;
  if (iterations < 1) return HG_EIDT_ITERATIONS;
  if (!(relaxation > 0.f && relaxation <= 1.f)) return HG_EIDT_RELAXATION;
  if (int rc = idt_check_pixels(n_src)) return rc;
  if (int rc = idt_check_pixels(n_tgt)) return rc;
  const IdtWorkspace w = idt_workspace(n_src, iterations, bins);
  if (workspace_bytes < w.total) return HG_EWORKSPACE;
  char *base = static_cast<char *>(workspace);
  float *planes = reinterpret_cast<float *>(base + w.planes), *map = reinterpret_cast<float *>(base + w.map);
  uint32_t *src_range = reinterpret_cast<uint32_t *>(base + w.src_range);
  uint32_t *tgt_range = reinterpret_cast<uint32_t *>(base + w.tgt_range);
  uint64_t *src_hist = reinterpret_cast<uint64_t *>(base + w.src_hist);
  uint64_t *tgt_hist = reinterpret_cast<uint64_t *>(base + w.tgt_hist);
  hipStream_t st = (hipStream_t)stream;
  int rc = idt_clear(src_range, 2, src_hist, 3LL * bins, st);
  if (!rc) rc = idt_clear(tgt_range, iterations, tgt_hist, (long long)iterations * 3 * bins, st);
  if (!rc) rc = idt_target_tables(target, n_tgt, tgt_pix_stride, tgt_chan_stride, rotations, iterations, bins, tgt_range,
                                  tgt_hist, st);
  if (!rc) rc = idt_range(source, n_src, src_pix_stride, src_chan_stride, rotations, 1, src_range, planes, st);
  const long long np = idt_plane_stride(n_src);
  for (int i = 0; i < iterations && !rc; ++i) {
    uint32_t *cur = src_range + 6 * (i & 1), *next = src_range + 6 * ((i + 1) & 1);
    const float *R = rotations + 9 * i;
    const bool last = i + 1 == iterations;
    rc = idt_hist(planes, n_src, 1, np, R, 1, bins, cur, src_hist, 0, st);
    if (!rc) rc = idt_table(src_hist, tgt_hist + (size_t)i * 3 * bins, tgt_range + 6 * i, bins, map, next, 1, st);
    if (!rc) rc = idt_apply(planes, n_src, R, last ? nullptr : R + 9, bins, cur, map, relaxation, next, out, out_u8, st);
  }
  return rc;
}

}  // extern "C"
