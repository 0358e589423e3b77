// hg_regrain.hip -- regrain (include/hg_regrain.h, hg_regrain_*): the gradient field of the original photo put back under the
// colours of a transferred picture, as a multi-level damped Jacobi solve on the offset field D = J - I.  The stages are
// elementwise (begin, coef, finish) but for the sweep, the hot path: one sweep per launch through global memory, or k sweeps per
// launch on a 64 x 64 tile and its halo held in LDS.  Both call rg_update, whose operations are spelled out, so they give the
// same bits.  The levels are composed by the caller (post.regrain) with the resize kernel of hg_post.hip in between.
#include "hg_host.h"
#include "../../include/hg_regrain.h"

namespace {

constexpr int RG_T = HG_REGRAIN_TILE;                  // the fused kernel's output tile, and 4 x the unfused block's width
constexpr int RG_THREADS = 256;                        // elementwise kernels and the unfused sweep (64 x 4 lanes of 4 pixels)
constexpr int RG_FUSED_THREADS = 1024;                 // one lane per 4 pixels of the 64 x 64 tile
constexpr int RG_PLANES = 6;                           // LDS: D twice, psi E, w_r, w_d, s
constexpr long long RG_MAX_PIXELS = 1LL << 28;
constexpr float RG_RHO = 0.2f;
constexpr float RG_ONE_MINUS_RHO = 1.0f - 0.2f;
constexpr int rg_halo_x(int k) { return (k + 3) / 4 * 4; }
static_assert(RG_T % 4 == 0 && RG_T * (RG_T / 4) == RG_FUSED_THREADS, "one lane per four pixels of the tile");
static_assert((size_t)(RG_T + 2 * HG_REGRAIN_MAX_FUSED) * (RG_T + 2 * rg_halo_x(HG_REGRAIN_MAX_FUSED)) * 4 * RG_PLANES <= 160 * 1024,
              "the staged region of the deepest fusion");

extern __shared__ f32x4 rg_lds[];

// The one update (include/hg_regrain.h, Sweep): pe = psi E; a missing neighbour comes with weight 0 and value 0.
__device__ __forceinline__ float rg_update(float pe, float s, float wr, float wl, float wd, float wu, float dc, float dr, float dl,
                                           float dd, float du) {
  float a = pe;
  a = fmaf(wr, dr, a);
  a = fmaf(wl, dl, a);
  a = fmaf(wd, dd, a);
  a = fmaf(wu, du, a);
  return fmaf(s, a, __fmul_rn(RG_RHO, dc));
}

// four cells of a row through rg_update: the neighbours inside the four come from the four, the two outside are dl (wl) and dr
__device__ __forceinline__ f32x4 rg_update4(f32x4 pe, f32x4 s, f32x4 wr, float wl, f32x4 wd, f32x4 wu, f32x4 dc, float dr, float dl,
                                            f32x4 dd, f32x4 du) {
  f32x4 o;
  o[0] = rg_update(pe[0], s[0], wr[0], wl, wd[0], wu[0], dc[0], dc[1], dl, dd[0], du[0]);
  o[1] = rg_update(pe[1], s[1], wr[1], wr[0], wd[1], wu[1], dc[1], dc[2], dc[0], dd[1], du[1]);
  o[2] = rg_update(pe[2], s[2], wr[2], wr[1], wd[2], wu[2], dc[2], dc[3], dc[1], dd[2], du[2]);
  o[3] = rg_update(pe[3], s[3], wr[3], wr[2], wd[3], wu[3], dc[3], dr, dc[2], dd[3], du[3]);
  return o;
}

__device__ __forceinline__ f32x4 rg_mul4(f32x4 a, f32x4 b) {
  f32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = __fmul_rn(a[k], b[k]);
  return o;
}

// cells x .. x + 3 of an image row (x >= 0, x % 4 == 0, x < W); 0 for the cells past the row's end, which are not addressed.
// VEC: W % 4 == 0 and the plane 16-byte aligned, so the four lie inside and the address is a multiple of 16.
template <bool VEC>
__device__ __forceinline__ f32x4 rg_ld4(const float *__restrict__ row, int x, int W) {
  if constexpr (VEC) {
    return *reinterpret_cast<const f32x4 *>(row + x);
  } else {
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = x + k < W ? row[x + k] : 0.f;
    return v;
  }
}

template <bool VEC>
__device__ __forceinline__ void rg_st4(float *__restrict__ row, int x, int W, f32x4 v) {
  if constexpr (VEC) {
    *reinterpret_cast<f32x4 *>(row + x) = v;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x + k < W) row[x + k] = v[k];
  }
}

__device__ __forceinline__ f32x4 rg_zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// ---- begin / finish -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_THREADS) void k_rg_begin(const float *__restrict__ o, long long ops, long long ocs,
                                                         const float *__restrict__ t, long long tps, long long tcs, long long n,
                                                         float *__restrict__ I, float *__restrict__ E) {
  const long long p = (long long)blockIdx.x * RG_THREADS + threadIdx.x;
  if (p >= n) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float iv = o[p * ops + c * ocs], tv = t[p * tps + c * tcs];
    I[c * n + p] = iv;
    E[c * n + p] = __fsub_rn(tv, iv);
  }
}

template <bool U8>
__global__ __launch_bounds__(RG_THREADS) void k_rg_finish(const float *__restrict__ I, const float *__restrict__ D, long long n,
                                                          void *__restrict__ out) {
  const long long p = (long long)blockIdx.x * RG_THREADS + threadIdx.x;
  if (p >= n) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = hg_clamp01(__fadd_rn(I[c * n + p], D[c * n + p]));
    if constexpr (U8) static_cast<uint8_t *>(out)[3 * p + c] = (uint8_t)__fmul_rn(v, 255.f);
    else static_cast<float *>(out)[3 * p + c] = v;
  }
}

// ---- coefficients ---------------------------------------------------------------------------------------------------------
// pass 1: psi into coef plane 0, phi into scratch
__global__ __launch_bounds__(RG_THREADS) void k_rg_phi(const float *__restrict__ I, int H, int W, float base, float smooth,
                                                       float *__restrict__ psi, float *__restrict__ phi) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const size_t hw = (size_t)H * W, p = (size_t)y * W + x;
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float *pl = I + c * hw + p;
    const float v = pl[0];
    const float gx = x + 1 < W ? __fsub_rn(pl[1], v) : 0.f;
    const float gy = y + 1 < H ? __fsub_rn(pl[W], v) : 0.f;
    q = c == 0 ? __fmul_rn(gx, gx) : __fadd_rn(q, __fmul_rn(gx, gx));
    q = __fadd_rn(q, __fmul_rn(gy, gy));
  }
  const float d = __fsqrt_rn(q);
  psi[p] = fminf(1.f, __fdiv_rn(__fmul_rn(256.f, d), 5.f));
  phi[p] = __fdiv_rn(base, __fadd_rn(1.f, __fdiv_rn(__fmul_rn(10.f, d), smooth)));
}

// pass 2: w_r, w_d and s from phi and psi
__global__ __launch_bounds__(RG_THREADS) void k_rg_weights(const float *__restrict__ phi, int H, int W, float *__restrict__ coef) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const size_t hw = (size_t)H * W, p = (size_t)y * W + x;
  const float f = phi[p];
  const float wr = x + 1 < W ? __fmul_rn(0.5f, __fadd_rn(f, phi[p + 1])) : 0.f;
  const float wl = x > 0 ? __fmul_rn(0.5f, __fadd_rn(phi[p - 1], f)) : 0.f;
  const float wd = y + 1 < H ? __fmul_rn(0.5f, __fadd_rn(f, phi[p + W])) : 0.f;
  const float wu = y > 0 ? __fmul_rn(0.5f, __fadd_rn(phi[p - W], f)) : 0.f;
  const float den = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(coef[p], wr), wl), wd), wu);
  coef[hw + p] = wr;
  coef[2 * hw + p] = wd;
  coef[3 * hw + p] = __fdiv_rn(RG_ONE_MINUS_RHO, den);
}

// ---- the sweep, one per launch ----------------------------------------------------------------------------------------------
// grid (ceil(W / 256), ceil(H / 4), 3), 64 x 4 lanes, a lane takes cells x .. x + 3 of row y of channel blockIdx.z
template <bool VEC>
__global__ __launch_bounds__(RG_THREADS) void k_rg_sweep(const float *__restrict__ Din, float *__restrict__ Dout,
                                                         const float *__restrict__ E, const float *__restrict__ coef, int H, int W) {
  const int x = 4 * (blockIdx.x * 64 + (threadIdx.x & 63)), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const size_t hw = (size_t)H * W, row = (size_t)y * W, ch = blockIdx.z * hw;
  const float *d = Din + ch + row, *wr = coef + hw + row, *wd = coef + 2 * hw + row;
  const f32x4 dc = rg_ld4<VEC>(d, x, W);
  const f32x4 pe = rg_mul4(rg_ld4<VEC>(coef + row, x, W), rg_ld4<VEC>(E + ch + row, x, W));
  const f32x4 r = rg_ld4<VEC>(wr, x, W), dn = rg_ld4<VEC>(wd, x, W), s = rg_ld4<VEC>(coef + 3 * hw + row, x, W);
  f32x4 du = rg_zero4(), wu = rg_zero4(), dd = rg_zero4();
  float dl = 0.f, wl = 0.f, dr = 0.f;
  if (y > 0) {
    du = rg_ld4<VEC>(d - W, x, W);
    wu = rg_ld4<VEC>(wd - W, x, W);
  }
  if (y + 1 < H) dd = rg_ld4<VEC>(d + W, x, W);
  if (x > 0) {
    dl = d[x - 1];
    wl = wr[x - 1];
  }
  if (x + 4 < W) dr = d[x + 4];
  rg_st4<VEC>(Dout + ch + row, x, W, rg_update4(pe, s, r, wl, dn, wu, dc, dr, dl, dd, du));
}

// ---- the sweep, `sweeps` per launch on a tile in LDS --------------------------------------------------------------------------
// grid (ceil(W / 64), ceil(H / 64), 3).  The region is the tile and a halo of hy rows and hx = a multiple of 4 columns, RH x RW
// cells = RH x RW4 groups of four; cell (ry, 4 g + j) of the region is pixel (y0 + ry, x0 + 4 g + j), and x0 % 4 == 0.  Cells
// outside the image hold zeros in all planes and are never loaded; a group on the region's border takes 0 for the neighbours
// the region does not hold (such a cell is the image's own border, or lies in the halo that `sweeps` <= hy, hx sweeps spoil).
template <bool VEC>
__global__ __launch_bounds__(RG_FUSED_THREADS) void k_rg_fused(const float *__restrict__ Din, float *__restrict__ Dout,
                                                               const float *__restrict__ E, const float *__restrict__ coef, int H,
                                                               int W, int sweeps, int hx, int hy) {
  const int RW4 = (RG_T + 2 * hx) / 4, RH = RG_T + 2 * hy, cells4 = RH * RW4;
  f32x4 *P0 = rg_lds, *P1 = P0 + cells4, *PE = P1 + cells4, *WR = PE + cells4, *WD = WR + cells4, *S = WD + cells4;
  const int x0 = blockIdx.x * RG_T - hx, y0 = blockIdx.y * RG_T - hy;
  const size_t hw = (size_t)H * W, ch = blockIdx.z * hw;
  for (int i = threadIdx.x; i < cells4; i += RG_FUSED_THREADS) {
    const int ry = i / RW4, g = i - ry * RW4, y = y0 + ry, x = x0 + 4 * g;
    f32x4 d = rg_zero4(), pe = d, r = d, dn = d, s = d;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const size_t row = (size_t)y * W;
      d = rg_ld4<VEC>(Din + ch + row, x, W);
      pe = rg_mul4(rg_ld4<VEC>(coef + row, x, W), rg_ld4<VEC>(E + ch + row, x, W));
      r = rg_ld4<VEC>(coef + hw + row, x, W);
      dn = rg_ld4<VEC>(coef + 2 * hw + row, x, W);
      s = rg_ld4<VEC>(coef + 3 * hw + row, x, W);
    }
    P0[i] = d;
    PE[i] = pe;
    WR[i] = r;
    WD[i] = dn;
    S[i] = s;
  }
  __syncthreads();
  f32x4 *src = P0, *dst = P1;
  for (int it = 0; it < sweeps; ++it) {
    const float *srcf = reinterpret_cast<const float *>(src), *wrf = reinterpret_cast<const float *>(WR);
    for (int i = threadIdx.x; i < cells4; i += RG_FUSED_THREADS) {
      const int ry = i / RW4, g = i - ry * RW4;
      f32x4 du = rg_zero4(), wu = du, dd = du;
      float dl = 0.f, wl = 0.f, dr = 0.f;
      if (ry > 0) {
        du = src[i - RW4];
        wu = WD[i - RW4];
      }
      if (ry + 1 < RH) dd = src[i + RW4];
      if (g > 0) {
        dl = srcf[4 * i - 1];
        wl = wrf[4 * i - 1];
      }
      if (g + 1 < RW4) dr = srcf[4 * i + 4];
      dst[i] = rg_update4(PE[i], S[i], WR[i], wl, WD[i], wu, src[i], dr, dl, dd, du);
    }
    __syncthreads();
    f32x4 *t = src;
    src = dst;
    dst = t;
  }
  const int ty = threadIdx.x / (RG_T / 4), tg = threadIdx.x - ty * (RG_T / 4);
  const int y = blockIdx.y * RG_T + ty, x = blockIdx.x * RG_T + 4 * tg;
  if (y < H && x < W) rg_st4<VEC>(Dout + ch + (size_t)y * W, x, W, src[(ty + hy) * RW4 + hx / 4 + tg]);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
bool rg_aligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }
int rg_check_size(int H, int W) { return H < 2 || W < 2 || (long long)H * W > RG_MAX_PIXELS ? HG_EREGRAIN_SIZE : HG_OK; }
int rg_check_smoothness(double s) { return s > 0.0 && s < INFINITY && (float)s > 0.f && (float)s < INFINITY ? HG_OK : HG_EREGRAIN_SMOOTHNESS; }
size_t rg_up4(size_t floats) { return (floats + 3) / 4 * 4; }
bool rg_overlap(const float *a, size_t na, const float *b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb * sizeof(float) && b0 < a0 + na * sizeof(float);
}

int rg_levels(int H, int W, int n_iterations, int min_side) {
  int levels = 1;
  while (levels < n_iterations && levels <= HG_REGRAIN_MAX_LEVEL) {
    H = (H + 1) / 2;
    W = (W + 1) / 2;
    if (H <= min_side || W <= min_side) break;
    ++levels;
  }
  return levels;
}

// Measured on one MI355X (tools/regrain_probe.py), which setting ran n sweeps on an H x W level faster:
// from 32 x 32 to 3000 x 4000 the tiled kernel won wherever it took n >= 4 sweeps in the fewest launches with the smallest
// halo -- 4 at n = 4 (8 was 3 % slower: the same launch, a wider halo), 8 at n = 16, 32, 64 (1.4 to 2.3 x the speed of one
// sweep per launch).  Two sweeps per launch lost to one at 750 x 1000 and below, and n < 4 was not measured: one per launch.
int rg_plan_fused(int H, int W, int n) {
  (void)H;
  (void)W;
  return n < 4 ? 1 : (n < HG_REGRAIN_MAX_FUSED ? n : HG_REGRAIN_MAX_FUSED);
}

dim3 rg_grid_px(int H, int W) { return dim3((W + 63) / 64, (H + 3) / 4); }

}  // namespace

extern "C" {

int hg_regrain_tile_h(void) { return RG_T; }
int hg_regrain_tile_w(void) { return RG_T; }
int hg_regrain_max_fused(void) { return HG_REGRAIN_MAX_FUSED; }
int hg_regrain_plan_fused(int32_t H, int32_t W, int32_t n) { return rg_check_size(H, W) || n < 1 ? 0 : rg_plan_fused(H, W, n); }
int hg_regrain_sweep_launches(int32_t n, int32_t fused) {
  return n < 1 || fused < 1 || fused > HG_REGRAIN_MAX_FUSED ? 0 : (n + fused - 1) / fused;
}

int hg_regrain_check(int32_t H, int32_t W, int32_t n_iterations, double smoothness, int32_t min_side) {
  if (int rc = rg_check_size(H, W)) return rc;
  if (n_iterations < 1) return HG_EREGRAIN_ITERATIONS;
  if (int rc = rg_check_smoothness(smoothness)) return rc;
  return min_side < 1 ? HG_EREGRAIN_MIN_SIDE : HG_OK;
}

int hg_regrain_levels(int32_t H, int32_t W, int32_t n_iterations, int32_t min_side) {
  return rg_check_size(H, W) || n_iterations < 1 || min_side < 1 ? 0 : rg_levels(H, W, n_iterations, min_side);
}

size_t hg_regrain_workspace_bytes(int32_t H, int32_t W, int32_t levels) {
  if (rg_check_size(H, W) || levels < 1 || levels > HG_REGRAIN_MAX_LEVEL + 1) return 0;
  size_t floats = 0;
  for (int l = 0; l < levels; ++l) {
    if (H < 2 || W < 2) return 0;
    const size_t hw = (size_t)H * W;
    floats += 4 * rg_up4(3 * hw) + rg_up4(4 * hw) + rg_up4(hw);
    H = (H + 1) / 2;
    W = (W + 1) / 2;
  }
  return floats * sizeof(float);
}

int hg_regrain_begin(const float *original, int64_t o_pix_stride, int64_t o_chan_stride, const float *transferred,
                     int64_t t_pix_stride, int64_t t_chan_stride, int32_t H, int32_t W, float *I, float *E, void *stream) {
  if (!original || !transferred || !I || !E || o_pix_stride <= 0 || o_chan_stride <= 0 || t_pix_stride <= 0 || t_chan_stride <= 0 ||
      !rg_aligned(original, 3) || !rg_aligned(transferred, 3) || !rg_aligned(I, 3) || !rg_aligned(E, 3))
    return HG_EINVAL;
  if (int rc = rg_check_size(H, W)) return rc;
  const long long n = (long long)H * W;
  if (rg_overlap(I, 3 * n, E, 3 * n)) return HG_EINVAL;
  return launch(k_rg_begin, dim3((unsigned)((n + RG_THREADS - 1) / RG_THREADS)), dim3(RG_THREADS), 0, (hipStream_t)stream, original,
                o_pix_stride, o_chan_stride, transferred, t_pix_stride, t_chan_stride, n, I, E);
}

int hg_regrain_coef(const float *I, int32_t H, int32_t W, int32_t level, double smoothness, float *coef, float *scratch,
                    void *stream) {
  if (!I || !coef || !scratch || level < 0 || level > HG_REGRAIN_MAX_LEVEL || !rg_aligned(I, 3) || !rg_aligned(coef, 3) ||
      !rg_aligned(scratch, 3))
    return HG_EINVAL;
  if (int rc = rg_check_size(H, W)) return rc;
  if (int rc = rg_check_smoothness(smoothness)) return rc;
  const size_t hw = (size_t)H * W;
  if (rg_overlap(coef, 4 * hw, scratch, hw) || rg_overlap(coef, 4 * hw, I, 3 * hw) || rg_overlap(scratch, hw, I, 3 * hw)) return HG_EINVAL;
  const dim3 grid = rg_grid_px(H, W);
  if (!grid_ok(grid.x, grid.y, 1)) return HG_EREGRAIN_SIZE;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch(k_rg_phi, grid, dim3(RG_THREADS), 0, st, I, H, W, ldexpf(30.f, -level), (float)smoothness, coef, scratch)) return rc;
  return launch(k_rg_weights, grid, dim3(RG_THREADS), 0, st, (const float *)scratch, H, W, coef);
}

int hg_regrain_sweep(float *a, float *b, const float *E, const float *coef, int32_t H, int32_t W, int32_t n, int32_t fused,
                     void *stream) {
  if (!a || !b || !E || !coef || fused < 0 || fused > HG_REGRAIN_MAX_FUSED || !rg_aligned(a, 3) || !rg_aligned(b, 3) ||
      !rg_aligned(E, 3) || !rg_aligned(coef, 3))
    return HG_EINVAL;
  if (int rc = rg_check_size(H, W)) return rc;
  if (n < 1) return HG_EREGRAIN_ITERATIONS;
  const size_t hw = (size_t)H * W;
  if (rg_overlap(a, 3 * hw, b, 3 * hw) || rg_overlap(a, 3 * hw, E, 3 * hw) || rg_overlap(b, 3 * hw, E, 3 * hw) ||
      rg_overlap(a, 3 * hw, coef, 4 * hw) || rg_overlap(b, 3 * hw, coef, 4 * hw))
    return HG_EINVAL;
  const int k = fused ? fused : rg_plan_fused(H, W, n);
  const bool vec = W % 4 == 0 && rg_aligned(a, 15) && rg_aligned(b, 15) && rg_aligned(E, 15) && rg_aligned(coef, 15);
  hipStream_t st = (hipStream_t)stream;
  const float *src = a;
  float *dst = b;
  if (k == 1) {
    const dim3 grid((W + 4 * 64 - 1) / (4 * 64), (H + 3) / 4, 3);
    if (!grid_ok(grid.x, grid.y, grid.z)) return HG_EREGRAIN_SIZE;
    for (int it = 0; it < n; ++it) {
      if (int rc = dispatch([&](auto VEC) { return launch(k_rg_sweep<VEC>, grid, dim3(RG_THREADS), 0, st, src, dst, E, coef, H, W); }, vec))
        return rc;
      float *t = const_cast<float *>(src);
      src = dst;
      dst = t;
    }
    return HG_OK;
  }
  const int hx = rg_halo_x(k), hy = k;
  const size_t lds = (size_t)(RG_T + 2 * hy) * (RG_T + 2 * hx) * sizeof(float) * RG_PLANES;
  const dim3 grid((W + RG_T - 1) / RG_T, (H + RG_T - 1) / RG_T, 3);
  if (!grid_ok(grid.x, grid.y, grid.z)) return HG_EREGRAIN_SIZE;
  for (int done = 0; done < n; done += k) {
    const int sweeps = n - done < k ? n - done : k;
    if (int rc = dispatch([&](auto VEC) {
          return launch(k_rg_fused<VEC>, grid, dim3(RG_FUSED_THREADS), lds, st, src, dst, E, coef, H, W, sweeps, hx, hy);
        }, vec))
      return rc;
    float *t = const_cast<float *>(src);
    src = dst;
    dst = t;
  }
  return HG_OK;
}

int hg_regrain_finish(const float *I, const float *D, int32_t H, int32_t W, void *out, int32_t quantize, void *stream) {
  if (!I || !D || !out || !rg_aligned(I, 3) || !rg_aligned(D, 3) || !rg_aligned(out, quantize ? 0 : 3)) return HG_EINVAL;
  if (int rc = rg_check_size(H, W)) return rc;
  const long long n = (long long)H * W;
  const dim3 grid((unsigned)((n + RG_THREADS - 1) / RG_THREADS));
  hipStream_t st = (hipStream_t)stream;
  return dispatch([&](auto U8) { return launch(k_rg_finish<U8>, grid, dim3(RG_THREADS), 0, st, I, D, n, out); }, quantize != 0);
}

}  // extern "C"
