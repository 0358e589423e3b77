/* hg_regrain.h -- C ABI of regrain, the edge-aware gradient restoration after a colour transfer (libhistogan_hip.so, since
 * version 117; no code of the reference, which has none).  The second half of Pitie, Kokaram, Dahyot 2007, "Automated colour
 * grading using colour distribution transfer": the result keeps the colours of the transferred picture T and takes the
 * gradient field of the original I, which removes the grain and the stretched compression blocks a distribution transfer
 * leaves on flat regions.
 *
 *   hg_regrain_begin    I and T as (H, W, 3) views -> the fp32 planes I (3) and E = T - I (3)
 *   hg_regrain_coef     a level's I planes -> the four coefficient planes the sweep reads
 *   hg_regrain_sweep    n damped Jacobi sweeps on a level, one per launch or k per launch on a tile staged in LDS
 *   hg_regrain_finish   clip(I + D, 0, 1) as (H, W, 3) fp32 or uint8
 *
 * Conventions as in hg_hist.h and hg_post.h: return 0 / negative HG_E* / positive hipError_t; device pointers; enqueue on
 * `stream`; never allocate or synchronise; nothing is launched for invalid arguments.  Pixels of a view are addressed as in
 * hg_color_moments: pixel p = y W + x, channel c at x[p*pix_stride + c*chan_stride] (HWC: 3, 1; a CHW image: 1, H W).
 * "Planes" are contiguous fp32 (C, H, W) stacks, plane c at base + c H W, 4-byte aligned; where W is a multiple of 4 and the
 * base is 16-byte aligned the kernels move 16 bytes per access, otherwise 4.
 *
 * Definition.  I the original, T the transferred picture, both (H, W, 3), H, W >= 2, E = T - I.  The output is
 *   J = clip(I + D_0, 0, 1), D_0 the level-0 result of the cascade below.  The unknown is the OFFSET field D = J - I, not the
 *   picture: the energy and its fixed point are the paper's, but T = I gives E = 0, D = 0 and J = I exactly, and T = I + c gives
 *   J = I + c up to rounding, at any number of sweeps.
 * Levels.  Level l has H_l x W_l pixels, H_{l+1} = ceil(H_l / 2), W likewise.  iterations = (n_0, n_1, ...); level l + 1 exists
 *   while iterations has an entry for it and both H_{l+1} and W_{l+1} exceed min_side (>= 1, so every level has H, W >= 2).
 *   hg_regrain_levels(H, W, n_iterations, min_side) = the number of levels (>= 1), 0 for refused arguments.
 *   I_{l+1} and E_{l+1} are the antialiased bilinear resize (hg_resize_axis, hg_post.h, post.imresize(method='bilinear')) of
 *   level l's planes.  The coarsest level starts from D = E_l, every other from D = the bilinear resize of D_{l+1} to H_l x W_l.
 * Coefficients of a level, from I_l alone (fp32, every operation rounded to nearest, no fused multiply-add, in this order):
 *     gx_c(x, y) = I_c(x+1, y) - I_c(x, y), 0 in the last column;  gy_c(x, y) = I_c(x, y+1) - I_c(x, y), 0 in the last row
 *     q = ((((gx_0 gx_0 + gy_0 gy_0) + gx_1 gx_1) + gy_1 gy_1) + gx_2 gx_2) + gy_2 gy_2;   d = sqrt(q)
 *     psi = min(1, (256 d) / 5)                                        the data weight
 *     phi = (30 2^-l) / (1 + (10 d) / smoothness)                      the smoothness weight (30 2^-l is exact; smoothness as fp32)
 *     w_r(x, y) = (phi(x, y) + phi(x+1, y)) / 2, 0 in the last column;  w_d(x, y) = (phi(x, y) + phi(x, y+1)) / 2, 0 in the last row
 *     w_l(x, y) = w_r(x-1, y), w_u(x, y) = w_d(x, y-1), 0 where the neighbour does not exist
 *     den = (((psi + w_r) + w_l) + w_d) + w_u      (> 0: H, W >= 2 give every pixel a neighbour, and phi > 0)
 *     s = (1 - rho) / den, rho = 1/5 rounded to fp32, 1 - rho rounded to fp32
 *   hg_regrain_coef writes coef = the planes (psi, w_r, w_d, s), fp32 (4, H, W), in two launches: phi into `scratch` (H W
 *   floats, distinct from coef), then the four planes.
 * Sweep.  Damped Jacobi, n_l times, every channel c on its own:
 *     D'(p) = s(p) (psi(p) E(p) + w_r D(right) + w_l D(left) + w_d D(down) + w_u D(up)) + rho D(p)
 *   which is D' = (1 - rho) (psi E + sum_q w_pq D(q)) / den + rho D.  In fp32, as ONE device function both kernels call:
 *     a = psi E;  a = fma(w_r, D(right), a);  a = fma(w_l, D(left), a);  a = fma(w_d, D(down), a);  a = fma(w_u, D(up), a);
 *     D' = fma(s, a, rho D)
 *   with weight 0 and value 0 for a neighbour outside the image: such a cell is never addressed, in global memory or in LDS.
 *   Every D' is computed from the previous D: source and destination are distinct buffers, so the result depends on no order
 *   and no tiling, and the fused and unfused kernels give the same bits.
 *   hg_regrain_sweep(a, b, ...): D is read from a; launch 1 writes b, launch 2 writes a, and so on, so the result is in b when
 *   hg_regrain_sweep_launches(n, fused) is odd and in a when it is even.  a and b are (3, H, W) planes that do not overlap.
 *   fused == 1: one sweep per launch, a lane takes 4 pixels of a row.
 *   fused == k, 2 <= k <= hg_regrain_max_fused() = 8: a workgroup of 1024 threads takes one channel of a tile of
 *     hg_regrain_tile_h() x hg_regrain_tile_w() = 64 x 64 pixels; it stages the tile and a halo of k rows above and below and
 *     4 ceil(k / 4) columns left and right (so that every row of the region starts on a 16-byte boundary) -- D twice, psi E,
 *     w_r, w_d, s: six planes of fp32 in LDS, at most 80 x 80 x 24 B = 153 600 B of the 160 KiB -- runs min(k, sweeps left)
 *     sweeps there on the whole region, and writes the tile.  A cell at distance j from the region's border is exact for the
 *     first j sweeps, the tile lies k or more inside, and the border cells are those of the image wherever the region reaches
 *     past it (the cells outside are zero in LDS and are never loaded).  A lane takes 4 consecutive cells of a row, so every
 *     LDS plane is read and written 16 bytes per lane (consecutive lanes on consecutive 16-byte slots: no bank conflict) but for
 *     the three single cells left and right of the four.  Launches: ceil(n / k).
 *   fused == 0 takes hg_regrain_plan_fused(H, W, n), the setting that measured faster: min(n, 8) from n = 4
 *     on, at every level size measured (32 x 32 to 3000 x 4000), and 1 below.
 * Finish.  J = clip(I + D, 0, 1) from the level-0 planes into (H, W, 3) contiguous fp32, or uint8 = (uint8)(v * 255)
 *   (truncation) when quantize != 0, as hg_color_affine.
 * Workspace.  hg_regrain_workspace_bytes(H, W, levels): per level, in this order and each rounded up to 16 bytes, the planes
 *   I (3), E (3), D a (3), D b (3), coef (4), scratch (1), level 0 first; what a composition of the stages across levels takes
 *   (post.regrain: on one stream, no host read-back).  0 for refused sizes.
 * Refusals, before any launch: a NULL or misaligned pointer, a non-positive stride, overlapping a and b, coef overlapping
 *   scratch, fused outside [0, 8], level outside [0, 30]: HG_EINVAL; H or W below 2, or H W above 2^28: HG_EREGRAIN_SIZE; n (or
 *   n_iterations) below 1: HG_EREGRAIN_ITERATIONS; a smoothness that is not positive and finite: HG_EREGRAIN_SMOOTHNESS;
 *   min_side below 1: HG_EREGRAIN_MIN_SIDE. */
#ifndef HG_REGRAIN_H
#define HG_REGRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HG_REGRAIN_MAX_FUSED 8
#define HG_REGRAIN_TILE 64
#define HG_REGRAIN_MAX_LEVEL 30

int hg_regrain_tile_h(void);
int hg_regrain_tile_w(void);
int hg_regrain_max_fused(void);
int hg_regrain_plan_fused(int32_t H, int32_t W, int32_t n);
int hg_regrain_sweep_launches(int32_t n, int32_t fused);
int hg_regrain_levels(int32_t H, int32_t W, int32_t n_iterations, int32_t min_side);
int hg_regrain_check(int32_t H, int32_t W, int32_t n_iterations, double smoothness, int32_t min_side);
size_t hg_regrain_workspace_bytes(int32_t H, int32_t W, int32_t levels);
int hg_regrain_begin(const float *original, int64_t o_pix_stride, int64_t o_chan_stride, const float *transferred,
                     int64_t t_pix_stride, int64_t t_chan_stride, int32_t H, int32_t W, float *I, float *E, void *stream);
int hg_regrain_coef(const float *I, int32_t H, int32_t W, int32_t level, double smoothness, float *coef, float *scratch,
                    void *stream);
int hg_regrain_sweep(float *a, float *b, const float *E, const float *coef, int32_t H, int32_t W, int32_t n, int32_t fused,
                     void *stream);
int hg_regrain_finish(const float *I, const float *D, int32_t H, int32_t W, void *out, int32_t quantize, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HG_REGRAIN_H */
