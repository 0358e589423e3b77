/* hg_lut.h -- C ABI of the 3D colour lookup tables (libhistogan_hip.so, since version 116; no code of the reference).
 *
 *   hg_lut_apply    a LUT applied to n pixels: tetrahedral or trilinear interpolation, one memory-bound pass
 *   hg_lut_splat    the integer normal sums of a fit from a pixel-paired source and target image
 *   hg_lut_solve    the smoothed, filled-in LUT from those sums: red-black Gauss-Seidel in fp64, one workgroup per channel
 *   hg_lut_fit      splat and solve on one stream, no read-back
 *   hg_lut_apply_bwd   (118) the adjoint of hg_lut_apply: the gradients for the pixels and for the LUT, integer sums again
 *   hg_lut_adam_step   (118) the gradient of a smoothness term and one Adam step on a LUT in one launch
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
 *   2^22 in the splat and the fit: HG_ELUT_PIXELS; a workspace below hg_lut_workspace_bytes: HG_EWORKSPACE.
 *
 * Backward of the apply (since version 118).  hg_lut_apply_bwd is the adjoint of hg_lut_apply for an fp32 source (x_u8 != 0 is
 *   refused: a uint8 source has no gradient), an fp32 output and the upstream gradient g, fp32 (n, 3) contiguous.  Either
 *   output may be NULL (not both): gx fp32 (n, 3) contiguous, glut fp32 (N, N, N, 3).  No mask is stored: per pixel the forward
 *   is recomputed with the sequence above (i, f, the sorted order, the nested fma / lerp), v_c = its value before the clip.
 *     m_c  = 1 iff 0 <= v_c <= 1 (the torch.clamp convention; a NaN v_c gives 0);   gm_c = m_c g_c, and a non-finite g_c is 0
 *     mx_c = 1 iff 0 <= x_c <= 1 on the value as given (NaN and +-inf give 0)
 *   gx, fp32, no reduction:  gx_c' = mx_c' (N - 1) S_c',  S_c' = fma(gm_2, s_2c', fma(gm_1, s_1c', fma(gm_0, s_0c', 0))), with
 *     s_cc' the slope of channel c along axis c' in the pixel's cell:
 *     tetrahedral: v1 - v0 along the axis of a, v2 - v1 along that of b, v3 - v2 along that of c (v_k = node c_k, channel c);
 *     trilinear: along r  lerp(lerp(d00, d10, f_g), lerp(d01, d11, f_g), f_b), d_jk = the node difference along r at (g + j, b + k);
 *                along g  lerp(e10 - e00, e11 - e01, f_b), e_jk the forward's lerps along r;  along b  h1 - h0, h_k = lerp(e0k, e1k, f_g).
 *   glut is a scatter: node j of the cell receives omega_j gm_c.  The nodes are the forward's (the order of the fp32 fractions);
 *     omega is fp64, from the unrounded fractions F_c = (double)x_c (N - 1) - i_c (exact), no contraction into fma:
 *     tetrahedral  1 - A, A - B, B - C, C on c0 .. c3 (A, B, C = F along the axes of a, b, c);
 *     trilinear  (wr wg) wb with w = (1 - F, F) per axis, on the eight corners.
 *     Nothing that is summed is a float.  gmax = the largest finite |g| (an integer atomic max over the bit patterns), E = the
 *     biased exponent field of gmax - 126 (so gmax < 2^E; a subnormal gmax takes E = -126), u = 2^(E - HG_LUT_GRAD_BITS),
 *       q = rint(omega_j * ((double)gm_c * 2^(36 - E)))      (the scaling is exact; the other products round as fp64 rounds)
 *     is added to an int64 counter per node and channel: in LDS up to N = hg_lut_grad_lds_n() = 17 (118 KB), flushed with 64-bit
 *     integer atomics, and in the global counters above.  glut = (float)((double)sum * u); gmax == 0 or no finite g at all gives
 *     glut = 0 without a read-back.  So glut has the same bits for every `blocks` and in every run.
 *     Bounds: omega <= 1 + 2^-17 (f can fall below 0 by 2^-24 N), so |q| <= 2^36 (1 + 2^-17) and with n <= hg_lut_grad_max_pixels()
 *     = 2^26 every |sum| < 2^63; a larger n is refused with HG_ELUT_PIXELS.  A node's error against the exact sum of its
 *     omega_j gm_c is at most count_j u / 2 (count_j = the contributions it received), u <= 2^-35 gmax, plus the roundings of
 *     the finish.
 *   workspace: hg_lut_grad_workspace_bytes(N) bytes, 16-byte aligned, needed when glut != NULL; the call clears it.  Afterwards
 *     it holds the bits of gmax (uint32 at byte 0) and the sums (int64 (N, N, N, 3) at byte 16).
 *   hg_lut_grad_blocks(n) = the workgroups of the plan (each a contiguous share of at least 4096 pixels, at most 256); `blocks`
 *     = 0 takes the plan, 1 .. 512 forces that count.  One stream: clear, range, scatter, finish; no read-back.
 * Adam step.  hg_lut_adam_step: lut_out = one Adam step of lut_in on grad + lambda dR/dlut, out of place (lut_in != lut_out;
 *   exp_avg, exp_avg_sq in place), fp32, no contraction into fma, per entry (node i, channel c):
 *     R(d) = (N - 1)^2 mean over the 3 N^2 (N - 1) lattice edges of |d_i - d_j|^2,   d = lut - identity, identity the fp32 value
 *       (float)((double)i_c / (N - 1));   coef = (float)(lambda 2 (N - 1)^2 / (3 N^2 (N - 1)))
 *     total = grad + coef ((float)deg_i d_i - nb_i)     nb_i, deg_i in the neighbour order of the solver (lambda == 0: total = grad)
 *     m = beta1 m + (1 - beta1) total;   v = beta2 v + ((1 - beta2) total) total
 *     lut_out = lut_in - (step_size m) / (sqrtf(v) rs + eps),  step_size = (float)(lr / (1 - beta1^step)),
 *       rs = (float)(1 / sqrt(1 - beta2^step)), both evaluated in fp64 on the host (torch.optim.Adam's update).
 * Refusals of the two: x_u8 != 0, a NULL g, both outputs NULL, blocks outside [0, 512], lut_in == lut_out, step < 1, a
 *   non-finite lr, a lambda or eps that is negative or not finite, a beta outside [0, 1): HG_EINVAL; N and the workspace as above;
 *   n above 2^26: HG_ELUT_PIXELS. */
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
#define HG_LUT_GRAD_BITS 36

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
int hg_lut_grad_lds_n(void);
int64_t hg_lut_grad_max_pixels(void);
int hg_lut_grad_blocks(int64_t n);
size_t hg_lut_grad_workspace_bytes(int32_t N);
int hg_lut_apply_bwd(const void *x, int32_t x_u8, int64_t n, int64_t pix_stride, int64_t chan_stride, const float *lut, int32_t N,
                     int32_t trilinear, const float *g, float *gx, float *glut, void *workspace, size_t workspace_bytes,
                     int32_t blocks, void *stream);
int hg_lut_adam_step(const float *lut_in, const float *grad, float *exp_avg, float *exp_avg_sq, float *lut_out, int32_t N,
                     double lambda, double lr, double beta1, double beta2, double eps, int32_t step, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HG_LUT_H */
