// hg_common.h -- shared device helpers for the gfx950 kernels (wave64, CDNA4).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define HG_WAVE 64

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#define HG_LAUNCH_CHECK()                          \
  do {                                             \
    hipError_t e__ = hipGetLastError();            \
    if (e__ != hipSuccess) return (int)e__;        \
  } while (0)

__device__ __forceinline__ float hg_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Block-wide sum for blockDim.x == 256 (4 waves); result valid in every thread.
__device__ __forceinline__ float hg_block_sum_256(float v, float *sm4 /* >= 4 floats of LDS */) {
  v = hg_wave_sum(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sm4[w] = v;
  __syncthreads();
  float r = (sm4[0] + sm4[1]) + (sm4[2] + sm4[3]);
  __syncthreads();
  return r;
}

// The same two in fp64: a fixed order, so repeats are bit-identical.
__device__ __forceinline__ double hg_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double hg_block_sum_256(double v, double *sm4 /* >= 4 doubles of LDS */) {
  v = hg_wave_sum(v);
  if ((threadIdx.x & 63) == 0) sm4[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = (sm4[0] + sm4[1]) + (sm4[2] + sm4[3]);
  __syncthreads();
  return r;
}

// Sum of n partials in a fixed order, blockDim.x == 256: thread t takes t, t + 256, ...; then the block sum.
__device__ __forceinline__ double hg_block_partials_sum_256(const double *__restrict__ part, int n, double *sm4) {
  double s = 0.0;
  for (int k = threadIdx.x; k < n; k += 256) s += part[k];
  return hg_block_sum_256(s, sm4);
}

__device__ __forceinline__ float hg_clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// Four packed RGB-u8 pixels, 12 bytes moved as three dwords (the address a multiple of 4); byte k of the 12 is
// component k % 3 of pixel k / 3.
struct alignas(4) HgBytes12 {
  uint32_t d[3];
};

// byte(k), k = 0 .. 11, gives the bytes by value: an array parameter would keep the caller's array in memory (k_idt_apply's
// tail also indexes it with a run-time k, and the array would go to scratch).
template <class F>
__device__ __forceinline__ HgBytes12 hg_pack_rgb4(F byte) {
  HgBytes12 v;
#pragma unroll
  for (int d = 0; d < 3; ++d)
    v.d[d] = (uint32_t)byte(4 * d) | ((uint32_t)byte(4 * d + 1) << 8) | ((uint32_t)byte(4 * d + 2) << 16) |
             ((uint32_t)byte(4 * d + 3) << 24);
  return v;
}

__device__ __forceinline__ void hg_unpack_rgb4(const HgBytes12 &v, uint8_t (&b)[12]) {
#pragma unroll
  for (int k = 0; k < 12; ++k) b[k] = (uint8_t)(v.d[k >> 2] >> (8 * (k & 3)));
}
