/* hg_lut.h -- C ABI of the 3D colour lookup tables (libhistogan_hip.so, since version 116; no code of the reference).
 *
 *   hg_lut_apply    a LUT applied to n pixels: tetrahedral or trilinear interpolation, one memory-bound pass
 *   hg_lut_splat    the integer normal sums of a fit from a pixel-paired source and target image
 *   hg_lut_solve    the smoothed, filled-in LUT from those sums: red-black Gauss-Seidel in fp64, one workgroup per channel
 *   hg_lut_fit      splat and solve on one stream, no read-back
 *
 * Conventions as in hg_hist.h and hg_post.h: return 0 / negative HG_E* / positive hipError_t; device pointers; enqueue on
 * `stream`; never allocate or synchronise; nothing is launched for invalid arguments.  Pixels are addressed as in
 * hg_color_moments: pixel p channel c at x[p*pix_stride + c*chan_stride] (HWC: 3, 1; planar: 1, n).
 *
 * A LUT is fp32 (N, N, N, 3), contiguous, indexed [b][g][r][c]: red is fastest, so the rows of lut as (N^3, 3) are the rows of
 *   a .cube file.  2 <= N <= hg_lut_max_n() = 65.  Its domain is [0, 1] on the sRGB-encoded values every other transfer takes:
 *   node (ir, ig, ib) holds the output colour for the input (ir, ig, ib) / (N - 1).  Entries are not clamped: an entry outside
 *   [0, 1] is representable (the network output is unclamped, and .cube allows it).
 *
 * Apply.  Per channel x = fminf(fmaxf(x, 0), 1): NaN reads as 0, -inf as 0, +inf as 1.  A uint8 source has x = v / 255 (fp32).
 *     i = min((int)(x (N - 1)), N - 2),   f = fma(x, N - 1, -i)
 *   so x == 1 reads cell N - 2 at f == 1 and no node N is ever read.  (The product that decides i is rounded to fp32, f is
 *   rounded once from the exact difference; where the rounded product reaches an integer the exact one stays just below, f is a
 *   negative number of the order of 2^-24 N: both interpolants are continuous across cells, so this moves nothing.)
 *   tetrahedral (trilinear == 0): the axes sorted by descending f, (a, A) >= (b, B) >= (c, C) with A, B, C the unit steps along
 *     them; c0 = the cell's corner (ir, ig, ib), c1 = c0 + A, c2 = c1 + B, c3 = c2 + C = the opposite corner;
 *       out = c0 + a (c1 - c0) + b (c2 - c1) + c (c3 - c2)
 *     four nodes.  On ties any order is allowed: the orders agree up to rounding.
 *   trilinear (trilinear != 0): the eight corners, lerp along r, then g, then b: lerp(u, v, f) = u + f (v - u).
 *   The output is clipped to [0, 1]: (n, 3) HWC contiguous, fp32 (16-byte aligned), or uint8 = (uint8)(v * 255) (truncation, 4-byte
 *   aligned) when out_u8 != 0, as hg_color_affine -- so an identity LUT on uint8 input is NOT an exact round trip: v / 255 * 255
 *   can land just below v and truncate to v - 1.
 *   Source forms: x_u8 == 0: fp32 with pix_stride, chan_stride > 0 (a packed HWC source, strides 3 and 1 and a 16-byte aligned
 *   base, is read 16 bytes at a time); x_u8 != 0: contiguous uint8 (n, 3), 4-byte aligned, strides ignored.  A batch of images
 *   with one LUT is a larger n.  A lane takes 4 pixels, a workgroup hg_lut_apply_tile() = 4096 at a time;
 *   hg_lut_apply_blocks(n) = the workgroups of the plan (at most 512, each walking tiles blocks apart); `blocks` = 0 takes the
 *   plan, 1 .. 512 forces that count -- the result has the same bits.  The LUT is staged in LDS up to N = hg_lut_apply_lds_n() =
 *   17 (59 KB) and read through the caches above.
 *
 * Fit.  Source image s, target image t, optional weight w, paired pixel by pixel; the unknown is the displacement
 *   d = LUT - identity on the lattice.  Everything that is summed is an integer, so no sum depends on its order and repeats are
 *   bit-identical.
 *   Fixed point, per pixel (fp64 on the fp32 inputs; every product below is exact in fp64, so rint sees exact values):
 *     x_c = clamp(s_c, 0, 1);   q_c = rint(x_c (N - 1) 2^5);   i_c = min(q_c >> 5, N - 2);   f_c = q_c - 32 i_c in [0, 32]
 *     qd_c = rint(clamp(t_c - x_c, -2, 2) 2^16)     (targets in [-1, 2] are covered: |t - x| <= 2)
 *     qw = rint(clamp(w, 0, 1) 2^8), 256 without a weight map
 *   A pixel with a non-finite component of s or t, or a non-finite w, is skipped (qw = 0).
 *   Splat.  The 8 corners j = (jr, jg, jb) in {0, 1}^3 of the cell (i_r, i_g, i_b) have the integer trilinear weights
 *     omega_j = prod_c (jc ? f_c : 32 - f_c), sum_j omega_j = 2^15; node i + j receives
 *       A += qw omega_j,      B_c += qw omega_j qd_c
 *     sums: int64 (N, N, N, 4) = (A, B_r, B_g, B_b) per node, indexed as the LUT, ADDED to what the caller left there.
 *     Bound: qw omega_j |qd_c| <= 2^8 2^15 2^17 = 2^40 per pixel and node, so with n <= hg_lut_max_pixels() = 2^22 pixel pairs
 *     every |sum| <= 2^62 < 2^63; a larger n is refused with HG_ELUT_PIXELS.  sum over the nodes of A = 2^15 sum_p qw exactly.
 *     A workgroup adds into 64-bit LDS counters up to N = hg_lut_splat_lds_n() = 17 (157 KB) and flushes them with 64-bit integer
 *     atomics; above it adds to the global counters directly.  There are no float atomics.  hg_lut_splat_blocks(n) = the
 *     workgroups of the plan (each a contiguous share of at least 4096 pixels, at most 256); `blocks` as in hg_lut_apply.
 *   Smooth and fill.  Per channel c, with S = sum over the nodes of A (integer) and scale = (double)N^3 / (double)S:
 *       a_i = (double)A_i scale        (mean 1 over the nodes, so lambda means the same at every N and image size)
 *       b_i = ((double)B_i scale) 2^-16
 *     solve (diag(a) + lambda L) d = b, L the 6-neighbour graph Laplacian of the lattice with natural boundaries (degree = the
 *     number of neighbours that exist).  Where data is, the data wins; where none is, d is the harmonic continuation of its
 *     surroundings.  S == 0 gives d = 0, the identity LUT: no read-back, no error.
 *   Solver.  From d = 0, `sweeps` red-black Gauss-Seidel sweeps in fp64, no fused multiply-add: per sweep first every node with
 *     (ir + ig + ib) even, then every node with it odd,
 *       d_i = (b_i + lambda nb_i) / (a_i + lambda deg_i)
 *     nb_i = the sum of d over the existing neighbours, added in the order r - 1, r + 1, g - 1, g + 1, b - 1, b + 1 starting from
 *     the first that exists.  The nodes of one colour do not read one another, so each half sweep is parallel and deterministic.
 *     With lambda == 0 a node without data (a_i == 0) keeps d_i = 0.  One workgroup per channel (the three are independent
 *     systems), a workgroup barrier between half sweeps, no barrier that spans workgroups and no atomics; d lives in LDS up to
 *     N = hg_lut_solve_lds_n() = 25 (125 KB of fp64) and in the workspace, which the L2 holds, above.
 *     LUT[ib][ig][ir][c] = (float)((double)i_c / (N - 1) + d_i), rounded once.
 *   hg_lut_workspace_bytes(N): the sums, the per-node (b, a + lambda deg) pairs and the global copy of d; 16-byte aligned; what
 *   hg_lut_fit and hg_lut_solve take (the solve leaves the part of the sums alone).  0 for a refused N.
 *   hg_lut_fit clears the sums in its workspace, splats and solves.
 * Refusals, before any launch: a NULL or misaligned pointer, a non-positive stride, n < 1, blocks outside [0, 512] (apply) or
 *   [0, 256] (splat), sweeps < 0, a lambda that is negative or not finite: HG_EINVAL; N outside [2, 65]: HG_ELUT_SIZE; n above
 *   2^22 in the splat and the fit: HG_ELUT_PIXELS; a workspace below hg_lut_workspace_bytes: HG_EWORKSPACE. */
#ifndef HG_LUT_H
#define HG_LUT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HG_LUT_MAX_N 65
#define HG_LUT_COORD_BITS 5
#define HG_LUT_WEIGHT_BITS 8
#define HG_LUT_DISP_BITS 16

int hg_lut_max_n(void);
int64_t hg_lut_max_pixels(void);
int hg_lut_apply_tile(void);
int hg_lut_apply_lds_n(void);
int hg_lut_splat_lds_n(void);
int hg_lut_solve_lds_n(void);
int hg_lut_apply_blocks(int64_t n);
int hg_lut_splat_blocks(int64_t n);
size_t hg_lut_workspace_bytes(int32_t N);
int hg_lut_apply(const void *x, int32_t x_u8, int64_t n, int64_t pix_stride, int64_t chan_stride, const float *lut, int32_t N,
                 int32_t trilinear, void *out, int32_t out_u8, int32_t blocks, void *stream);
int hg_lut_splat(const float *source, int64_t s_pix_stride, int64_t s_chan_stride, const float *target, int64_t t_pix_stride,
                 int64_t t_chan_stride, const float *weight, int64_t n, int32_t N, int64_t *sums, int32_t blocks, void *stream);
int hg_lut_solve(const int64_t *sums, int32_t N, double lambda, int32_t sweeps, float *lut, void *workspace,
                 size_t workspace_bytes, void *stream);
int hg_lut_fit(const float *source, int64_t s_pix_stride, int64_t s_chan_stride, const float *target, int64_t t_pix_stride,
               int64_t t_chan_stride, const float *weight, int64_t n, int32_t N, double lambda, int32_t sweeps, float *lut,
               void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HG_LUT_H */
