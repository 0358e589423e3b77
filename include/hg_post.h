/* hg_post.h -- C ABI of the full-resolution post-processing kernels (libhistogan_hip.so): the two ways the reference's
 * `rehistoGAN.py --generate` carries a 256x256 recoloured image back to the photo at its own resolution.
 *
 *   hg_resize_axis            MATLAB-style separable resize along one axis (utils/imresize.py:35-96): any tap count,
 *                             so down-scaling (kernel widened to 4/scale) is the same launch with a longer table
 *   hg_pyr_down               OpenCV pyrDown (5x5 binomial, every second row / column, BORDER_REFLECT_101)
 *   hg_pyr_up_add             one level of the Laplacian reconstruction of utils/pyramid_upsampling.py:74-85:
 *                             pyrUp(prev) + wa*(fineA - pyrUp(coarseA)) + wb*(fineB - pyrUp(coarseB)), the Laplacians
 *                             formed on the fly from the two Gaussian pyramids, never written
 *   hg_color_moments          per-image mean and unbiased 3x3 covariance (utils/color_transfer_MKL.py:13-14, 18-19), fp64
 *   hg_color_affine           (x - m0) T + m1, clipped to [0, 1], optionally quantised to uint8 by truncation (:20-25 and
 *                             the caller's np.uint8(result*255))
 *   hg_u8_hwc_to_f32          uint8 HWC -> fp32 planar, x/255 (torchvision ToTensor)
 *   hg_f32_to_u8_hwc          fp32 planar -> uint8 HWC, clamp(x*255 + 0.5, 0, 255) truncated (torchvision save_image)
 *   hg_srgb_to_lab            sRGB -> normalised CIE Lab (L/100, (a+128)/255, (b+128)/255): what LabHistBlock bins, for the
 *   hg_lab_to_srgb            reference README's "convert loaded images into the CIE LAB space", and its exact inverse
 *   hg_delta_e                CIE colour difference (dE76, CIEDE2000) of two sRGB images: per-sample mean, map and gradient
 *                             in one pass (no code of the reference: the perceptual colour term of a projection, and the dE
 *                             reported for recolourings)
 *   hg_ssim_fwd, hg_ssim_bwd  SSIM of two images (of their L* plane or of their components): per-sample means of ssim and cs,
 *                             map, pooled planes for the next MS-SSIM level; gradient by a second tiled pass (no code of the
 *                             reference: the structure term of a projection and of ReHistoGAN's reconstruction loss)
 *   hg_idt_run, hg_idt_*      iterative distribution transfer (Pitie, Kokaram, Dahyot 2007): the nonlinear colour transfer next
 *                             to hg_color_affine's linear one -- rotate the colour cloud, match the three 1-D marginals by
 *                             CDF matching, rotate back, repeat (no code of the reference, whose color_transfer_MKL.py took
 *                             the linear half of the same toolbox)
 *   hg_palette_run, hg_palette_*  an image described by K colours (integer k-means in Lab, seeded from a 16^3 grid), the
 *                             paired palette of two images, and hg_palette_transfer: every pixel moved by a smooth blend of
 *                             per-cluster shifts, the third transfer between the affine map and the distribution transfer
 *                             (no code of the reference)
 *
 * Conventions as in hg_hist.h: return 0 / negative HG_E* / positive hipError_t; device pointers unless stated; fp32;
 * enqueue on `stream`; never allocate or synchronise; nothing is launched for invalid arguments.  Planar images are
 * contiguous (C, H, W).  Every result is deterministic: no atomics, fixed reduction order (hg_idt_*, hg_palette_*: integer
 * atomics only, whose sums do not depend on their order).
 */
#ifndef HG_POST_H
#define HG_POST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Resize along one axis of a (C, H, W) image with arbitrary element strides (so uint8 HWC is xs = {1, W*C, C}):
 *   axis 0:  out[c, i, j] = sum_t weights[i*taps + t] * X[c, indices[i*taps + t], j]      out shape (C, out_len, W)
 *   axis 1:  out[c, i, j] = sum_t weights[j*taps + t] * X[c, i, indices[j*taps + t]]      out shape (C, H, out_len)
 * X = x as uint8 (x_u8 != 0) or fp32, clamped to [0, 1] first when clamp_in != 0.  Output uint8 (out_u8 != 0) is the
 * reference's np.around(np.clip(v, 0, 255)) (round half to even), fp32 otherwise.  weights (fp32) and indices (int32,
 * already folded into [0, in_len) by the host) are device tables of out_len x taps; an index outside [0, in_len) is
 * clamped to the edge rather than read.  Strides are in elements.  Requires taps >= 1, all sizes >= 1. */
int hg_resize_axis(const void *x, int32_t x_u8, int64_t xs_c, int64_t xs_h, int64_t xs_w, int32_t clamp_in, void *out,
                   int32_t out_u8, int64_t os_c, int64_t os_h, int64_t os_w, int32_t C, int32_t H, int32_t W,
                   int32_t axis, const float *weights, const int32_t *indices, int32_t out_len, int32_t taps,
                   void *stream);

/* out (C, (H+1)/2, (W+1)/2) = every second row and column of x (C, H, W) filtered with [1 4 6 4 1]^T [1 4 6 4 1] / 256,
 * source indices outside the image reflected without repeating the edge (BORDER_REFLECT_101: -1 -> 1, H -> H-2). */
int hg_pyr_down(const float *x, float *out, int32_t C, int32_t H, int32_t W, void *stream);

/* out (C, 2h, 2w) = U(prev) + wa * (fine_a - U(coarse_a)) + wb * (fine_b - U(coarse_b)),   prev, coarse_*: (C, h, w),
 * fine_*: (C, 2h, 2w).  U = OpenCV pyrUp: zeros inserted, [1 4 6 4 1]/8 per axis, i.e. per axis with source s[0..n-1]
 *   U[2i] = (s[i-1] + 6 s[i] + s[i+1]) / 8,   U[2i+1] = (s[i] + s[i+1]) / 2,   s[-1] = s[1], s[n] = s[n-1]
 * (reflect-101 at the left / top, replicate at the right / bottom).  A term whose weight is 0 is skipped and its two
 * pointers may be NULL; with wa = wb = 0 the call is a plain pyrUp of prev. */
int hg_pyr_up_add(const float *prev, const float *fine_a, const float *coarse_a, float wa, const float *fine_b,
                  const float *coarse_b, float wb, float *out, int32_t C, int32_t h, int32_t w, void *stream);

/* moments[0..2] = per-channel mean, moments[3..11] = the 3x3 covariance (row-major, divided by n - 1) of n 3-channel
 * pixels, pixel p channel c at x[p*pix_stride + c*chan_stride] (HWC: 3, 1; planar: 1, n).  fp64 device output;
 * accumulated in fp64 in two passes over per-block partials (workspace: hg_color_moments_workspace_bytes(n)).
 * Requires n >= 2. */
size_t hg_color_moments_workspace_bytes(int64_t n);
int hg_color_moments(const float *x, int64_t n, int64_t pix_stride, int64_t chan_stride, double *moments,
                     void *workspace, size_t workspace_bytes, void *stream);

/* out[p, :] = clip((x[p, :] - m0) T + m1, 0, 1) for n 3-channel pixels addressed as in hg_color_moments; out is HWC
 * (n, 3), fp32, or uint8 = (uint8)(v * 255) (truncation) when out_u8 != 0.  coef is a HOST array of 15 floats:
 * m0[3], T[9] (row-major), m1[3]. */
int hg_color_affine(const float *x, int64_t n, int64_t pix_stride, int64_t chan_stride, const float *coef, void *out,
                    int32_t out_u8, void *stream);

/* out (C, HW) fp32 = x (HW, C) uint8 / 255. */
int hg_u8_hwc_to_f32(const uint8_t *x, float *out, int32_t C, int64_t HW, void *stream);

/* out (HW, C) uint8 = (uint8) clamp(x * 255 + 0.5, 0, 255) of x (C, HW) fp32. */
int hg_f32_to_u8_hwc(const float *x, uint8_t *out, int32_t C, int64_t HW, void *stream);

/* Bilateral guided upsampling.  The grid has gh x gw x gd vertices, each a 3 x 4 affine colour model gamma[i][j]
 * (out_i = sum_j gamma[i][j] [r g b 1]_j).  Pixel (y, x) of an h x w image sits at cy = (y + 0.5)(gh - 1) / h,
 * cx = (x + 0.5)(gw - 1) / w, cz = (0.25 r + 0.5 g + 0.25 b)(gd - 1) and weighs the 8 vertices around it trilinearly; a
 * vertex outside the grid is dropped (luminance 1 has cz = gd - 1 and its upper vertex, of weight 0, is outside).
 * Requires 2 <= gh, gw <= 4096, 2 <= gd <= 64, image sides <= 2^24.
 *
 * hg_bgu_normal: the three output channels share one normal matrix N = A^T W A over the n = gh gw gd 4 unknowns
 * gamma[i][.] of a channel i.  Unknowns are ordered in S = max(gh, gw) slabs along the longer spatial axis (y when
 * gh >= gw), and within a slab as a = (t * gd + z) * 4 + j with t the index along the other axis (T = min(gh, gw)
 * vertices, m = T gd 4 unknowns per slab).  N is then block-tridiagonal:
 *   diag[s][a][b] = N[(s, a), (s, b)]            (S, m, m)   row-major fp64
 *   off [s][a][b] = N[(s + 1, a), (s, b)]        (S - 1, m, m)
 *   rhs [i][s][a] = (A^T W out_i)[(s, a)]        (3, S, m)
 * Every entry is written, the zeros between vertices more than 1 apart included.  in_ds, out_ds: fp32 planar (3, h, w);
 * weight: fp32 (h, w), non-negative, or NULL for ones.  Accumulated in fp64 in a fixed order (per floor cell, then the
 * up-to-four cells of a vertex pair), so repeats are bit-identical.  The smoothness terms are the caller's to add. */
size_t hg_bgu_normal_workspace_bytes(int32_t gh, int32_t gw, int32_t gd);
int hg_bgu_normal(const float *in_ds, const float *out_ds, const float *weight, int32_t h, int32_t w, int32_t gh,
                  int32_t gw, int32_t gd, double *diag, double *off, double *rhs, void *workspace,
                  size_t workspace_bytes, void *stream);

/* out = the grid sliced at every pixel of `photo` and applied to it.  gamma: fp32 (gh, gw, gd, 3, 4) row-major, i.e.
 * gamma[(((y * gw + x) * gd + z) * 3 + i) * 4 + j], 16-byte aligned.  photo: uint8 (H, W, 3) read as v / 255 with element
 * strides xs_h, xs_w, xs_c (rows of a packed photo, xs_w = 3 and xs_c = 1, are read 12 bytes at a time whatever xs_h
 * and W are).  out: uint8 (H, W, 3) contiguous = round(255 clip(v, 0, 1)), half away from zero (MATLAB imwrite of a
 * double image), when out_u8 != 0; fp32 planar (3, H, W), not clipped, otherwise.  HG_EUNSUPPORTED when the grid is so
 * fine against the photo (cells of about 6 pixels or fewer) that the vertices of a 256 x 4 pixel tile exceed 64 KiB of
 * LDS. */
int hg_bgu_slice(const float *gamma, int32_t gh, int32_t gw, int32_t gd, const uint8_t *photo, int64_t xs_h,
                 int64_t xs_w, int64_t xs_c, void *out, int32_t out_u8, int32_t H, int32_t W, void *stream);

/* sRGB <-> normalised CIE Lab (since version 107), the conversion HG_PROJ_LAB of hg_hist.h applies per pixel.  x: fp32
 * (B, 3, H, W) with element strides xs_*; out: fp32 (B, 3, H, W) contiguous.  Evaluated in fp64, rounded once to fp32.
 *   hg_srgb_to_lab: c = clamp(x, 0, 1); c_lin = c / 12.92 (c <= 0.04045) else ((c + 0.055) / 1.055)^2.4;
 *     (X, Y, Z) = M c_lin with M = [[0.412453 0.357580 0.180423] [0.212671 0.715160 0.072169] [0.019334 0.119193 0.950227]],
 *     every row divided by its own sum (D65 white = (1, 1, 1)); f(t) = cbrt(t) (t > (6/29)^3) else t / (3 (6/29)^2) + 4/29;
 *     L = 116 f(Y) - 16, a = 500 (f(X) - f(Y)), b = 200 (f(Y) - f(Z));  out = (L / 100, (a + 128) / 255, (b + 128) / 255).
 *   hg_lab_to_srgb: the exact inverse -- f^-1(s) = s^3 (s > 6/29) else 3 (6/29)^2 (s - 4/29), the inverse of the normalised
 *     matrix, c = 12.92 l (l <= 0.04045 / 12.92) else 1.055 l^(1/2.4) - 0.055 -- ending with a clip to [0, 1]. */
int hg_srgb_to_lab(const float *x, int64_t xs_b, int64_t xs_c, int64_t xs_h, int64_t xs_w, float *out, int32_t B,
                   int32_t H, int32_t W, void *stream);
int hg_lab_to_srgb(const float *x, int64_t xs_b, int64_t xs_c, int64_t xs_h, int64_t xs_w, float *out, int32_t B,
                   int32_t H, int32_t W, void *stream);

/* CIE colour difference between two sRGB images as a fused loss and metric (since version 110): the per-sample weighted
 * mean of dE, optionally the per-pixel dE and the gradient of the mean with respect to the first image, in one pass.
 *
 * Per pixel both images go through the chain of hg_srgb_to_lab above in fp64, on the fp32 inputs clamped to [0, 1], WITHOUT
 * the rounding to fp32 and without the 8-bit normalisation: L = 116 f(Y) - 16, a = 500 (f(X) - f(Y)), b = 200 (f(Y) - f(Z)).
 * Index 1 is the first image x1 (`pred`), index 2 the second x2 (`target`).
 *   kind = 76:    dE = sqrt(dL^2 + da^2 + db^2)
 *   kind = 2000:  CIEDE2000 (Sharma, Wu, Dalal 2005; kL = kC = kH = 1), angles in degrees:
 *     C_i = sqrt(a_i^2 + b_i^2), Cm = (C_1 + C_2) / 2
 *     G = (1 - sqrt(Cm^7 / (Cm^7 + 25^7))) / 2, a'_i = (1 + G) a_i, C'_i = sqrt(a'_i^2 + b_i^2)
 *     h'_i = atan2(b_i, a'_i) mapped into [0, 360), and 0 when C'_i = 0
 *     dh' = h'_2 - h'_1 brought into (-180, 180] by -+360; 0 when C'_1 C'_2 = 0
 *     dL' = L_2 - L_1, dC' = C'_2 - C'_1, dH' = 2 sqrt(C'_1 C'_2) sin(dh' / 2)
 *     Lm = (L_1 + L_2) / 2, Cm' = (C'_1 + C'_2) / 2
 *     hm' = (h'_1 + h'_2) / 2 when |h'_1 - h'_2| <= 180; otherwise (h'_1 + h'_2 + 360) / 2 when the sum is < 360, else
 *           (h'_1 + h'_2 - 360) / 2; when C'_1 C'_2 = 0, hm' = h'_1 + h'_2
 *     T = 1 - 0.17 cos(hm' - 30) + 0.24 cos(2 hm') + 0.32 cos(3 hm' + 6) - 0.20 cos(4 hm' - 63)
 *     dtheta = 30 exp(-((hm' - 275) / 25)^2), R_C = 2 sqrt(Cm'^7 / (Cm'^7 + 25^7))
 *     S_L = 1 + 0.015 (Lm - 50)^2 / sqrt(20 + (Lm - 50)^2), S_C = 1 + 0.045 Cm', S_H = 1 + 0.015 Cm' T
 *     R_T = -sin(2 dtheta) R_C
 *     dE = sqrt((dL'/S_L)^2 + (dC'/S_C)^2 + (dH'/S_H)^2 + R_T (dC'/S_C) (dH'/S_H))
 * Per sample b, with the optional map w (clamped to [0, 1] like hg_hist_params.weight; NULL = 1):
 *   mean[b] = sum_n w_n dE_n / sum_n w_n, and 0 when sum w = 0; summed in fp64 in a fixed order, rounded once.
 *   map[b, n] = dE_n (not weighted), rounded once.
 *   grad[b, c, n] = d mean[b] / d x1[b, c, n]: the partials of dE with respect to (L_1, a_1, b_1) pulled back through the
 *     Jacobian of the chain in fp64 and rounded once.  It is 0 for a component outside [0, 1] (the clamp's mask is
 *     inclusive, as aten's clamp backward).  A square root whose argument is 0 (dE = 0, C_i = 0, C'_i = 0) has slope 0, and
 *     so has atan2 at the origin; at a branch of dh' or hm' the slope is that of the branch the forward takes.  Hence grad
 *     is finite for every input, and x1 == x2 gives mean = 0 and grad = 0 (exactly: a pixel whose clamped components equal
 *     the other image's has dE = 0 and slope 0 by construction).  There is no gradient for x2 or w.
 * x1, x2: fp32 (B, 3, H, W), weight: fp32 (B, H, W), each with its own element strides; mean (B), map (B, H, W) and grad
 * (B, 3, H, W) are contiguous; map and grad may be NULL.  mean has the same bits whichever of map and grad are requested,
 * and a map of ones gives the bits of NULL.  workspace: hg_delta_e_workspace_bytes(B, H, W) bytes, 8-byte aligned.
 * HG_EINVAL before any launch for a NULL x1, x2, mean or workspace, a size < 1, B > 65535, more than 2^31 - 1 blocks of 256
 * pixels per image, a kind other than 76 and 2000, or a workspace that is too small (the query returns 0 for refused sizes). */
size_t hg_delta_e_workspace_bytes(int32_t B, int32_t H, int32_t W);
int hg_delta_e(const float *x1, int64_t s1_b, int64_t s1_c, int64_t s1_h, int64_t s1_w, const float *x2, int64_t s2_b,
               int64_t s2_c, int64_t s2_h, int64_t s2_w, const float *weight, int64_t ws_b, int64_t ws_h, int64_t ws_w,
               int32_t kind, float *mean, float *map, float *grad, int32_t B, int32_t H, int32_t W, void *workspace,
               size_t workspace_bytes, void *stream);

/* SSIM (and, level by level, MS-SSIM) of two images as a fused loss and metric (since version 111): per sample the mean of
 * ssim and the mean of cs, optionally the ssim map, and in a second call the gradient with respect to the first image.
 *
 * Planes.  mode HG_SSIM_L: x1, x2 are fp32 (B, 3, H, W) sRGB images with their own element strides, clamped to [0, 1] as they
 * are read; one plane, P = L / 100 with L = 116 f(Y) - 16 from the chain of hg_srgb_to_lab above in fp64, unrounded.
 * HG_SSIM_RGB: the same images, three planes, the clamped components.  HG_SSIM_PLANES1 / HG_SSIM_PLANES3: x1, x2 are
 * contiguous fp64 (B, 1 | 3, H, W) planes, taken as they are (the strides are ignored): the pooled planes of a coarser
 * MS-SSIM level.  x is the plane of x1 (`pred`), y that of x2 (`target`).
 * Window.  11 taps g_k = exp(-(k - 5)^2 / 4.5) / sum_k, fp64; the 2-D window is the outer product; only valid positions
 * count, so the map is (H - 10) x (W - 10) and H, W >= 11.
 * Per position, with the window means mx, my, exx, eyy, exy of x, y, x^2, y^2, x y:
 *   sxx = exx - mx^2, syy = eyy - my^2, sxy = exy - mx my;  C1 = 1e-4, C2 = 9e-4 (data range 1)
 *   A2 = mx^2 + my^2 + C1, B2 = sxx + syy + C2
 *   l = (2 mx my + C1) / A2,  cs = (2 sxy + C2) / B2,  ssim = l cs
 * hg_ssim_fwd:
 *   means[b] = (mean ssim, mean cs) over the N = (H - 10)(W - 10) * planes positions of sample b, fp64 (B, 2): block partials
 *     summed in a fixed order; the same bits whichever optional outputs are requested.
 *   map (optional): fp32 (B, H - 10, W - 10), ssim averaged over the planes in fp64, rounded once.
 *   pool1, pool2 (optional, both or neither): the planes of x1 and x2 averaged over 2 x 2 blocks, fp64 (B, planes, H/2, W/2)
 *     contiguous, an odd trailing row or column dropped (F.avg_pool2d(., 2)): the input of the next MS-SSIM level as
 *     HG_SSIM_PLANES*.  They stay fp64: a rounding to fp32 in front of exx - mx^2 would cost what the fp64 evaluation buys.
 *   workspace: hg_ssim_workspace_bytes(B, H, W) bytes, 8-byte aligned (the block partials).
 * hg_ssim_bwd: the gradient of  sum_b (a_b mean_ssim[b] + c_b mean_cs[b])  with respect to the planes of x1, coef = fp64
 *   (B, 2) = (a_b, c_b) in device memory.  With adj = the adjoint of the valid blur (zero-padded full correlation with g):
 *     dP = adj(M) + 2 x adj(Exx) + y adj(Exy)
 *     Exx = -(a l + c)(2 sxy + C2) / B2^2,  Exy = 2 (a l + c) / B2,
 *     M = a cs dl/dmx - 2 mx Exx - my Exy,  dl/dmx = 2 (my - l mx) / A2,      all three divided by N
 *   coarse (optional): fp64 (B, planes, H/2, W/2), the gradient of the pooled planes: 0.25 coarse[i/2, j/2] is added at every
 *     pixel a pooled pixel covers.
 *   grad: HG_SSIM_PLANES*: fp64 (B, planes, H, W), dP.  HG_SSIM_RGB: fp32 (B, 3, H, W), dP rounded once, 0 for a component
 *     outside [0, 1] (the clamp's inclusive mask).  HG_SSIM_L: fp32 (B, 3, H, W), dP / 100 pulled back through the Jacobian of
 *     the chain (as hg_delta_e), rounded once, with the same mask.
 *   Nothing is kept between the two calls: the moments are recomputed.  Denominators are at least C1 and C2, so the gradient
 *   is finite for every input; equal planes give ssim = 1 and gradient 0 exactly (l and cs are evaluated as 1 minus
 *   what separates them from 1 -- l = 1 - (mx - my)^2 / A2, cs = 1 - ((sxx - sxy) + (syy - sxy)) / B2 -- and the gradient's
 *   cancelling sums as differences that vanish term by term, so no contraction into fma's can leave a residue; in HG_SSIM_L
 *   equal clamped pixels give equal plane values by construction).  There is no
 *   gradient for x2.
 * MS-SSIM (composed by the caller, histogan_amd/post.py): five levels s, weights (0.0448, 0.2856, 0.3001, 0.2363, 0.1333),
 *   ms = prod_{s<5} max(mean cs_s, 0)^w_s * max(mean ssim_5, 0)^w_5 with slope 0 at the clamp; min(H, W) >= 176.
 * hg_ssim_tile(): the edge of a workgroup's tile (of the map in hg_ssim_fwd, of the input in hg_ssim_bwd);
 * hg_ssim_finish_threads(): the threads of the block that sums a sample's partials.
 * HG_EINVAL before any launch for a NULL x1, x2, means / coef / grad or workspace, only one of pool1 and pool2, H or W < 11,
 * B < 1 or > 65535, an unknown mode, or a workspace that is too small (the query returns 0 for refused sizes). */
#define HG_SSIM_L 0
#define HG_SSIM_RGB 1
#define HG_SSIM_PLANES1 2
#define HG_SSIM_PLANES3 3
#define HG_SSIM_TILE 32
#define HG_SSIM_FINISH_THREADS 256
int hg_ssim_tile(void);
int hg_ssim_finish_threads(void);
size_t hg_ssim_workspace_bytes(int32_t B, int32_t H, int32_t W);
int hg_ssim_fwd(const void *x1, int64_t s1_b, int64_t s1_c, int64_t s1_h, int64_t s1_w, const void *x2, int64_t s2_b,
                int64_t s2_c, int64_t s2_h, int64_t s2_w, int32_t mode, double *means, float *map, double *pool1,
                double *pool2, int32_t B, int32_t H, int32_t W, void *workspace, size_t workspace_bytes, void *stream);
int hg_ssim_bwd(const void *x1, int64_t s1_b, int64_t s1_c, int64_t s1_h, int64_t s1_w, const void *x2, int64_t s2_b,
                int64_t s2_c, int64_t s2_h, int64_t s2_w, int32_t mode, const double *coef, const double *coarse, void *grad,
                int32_t B, int32_t H, int32_t W, void *stream);

/* Iterative distribution transfer (since version 113).  Inputs: n_src source pixels x_j and n_tgt target pixels y_j (3
 * channels, addressed as in hg_color_moments; the two counts are independent), `iterations` rotations R_i (fp32 DEVICE array
 * (iterations, 3, 3) row-major, orthonormal, row a = axis a), bins = n >= 2 nodes and relaxation rho in (0, 1].  For every
 * rotation in order and every axis a independently:
 *   1. v_j = R_i[a] . x_j = fma(R[a][2], x2, fma(R[a][1], x1, R[a][0] x0)), [lo0, hi0] = min / max of v; likewise w_j,
 *      [lo1, hi1] for the target.
 *   2. Linear-binned fixed-point histogram over n nodes, the same rule for source and target over their own ranges:
 *      u = (v - lo) (n - 1) / (hi - lo) clamped to [0, n - 1], k = min(floor(u), n - 2), t = u - k, q = floor(t 65536 + 0.5);
 *      node k receives 65536 - q and node k + 1 receives q.  Every pixel deposits 65536 units: sum_k h[k] == 65536 N exactly.
 *      On an axis with !(hi - lo > 2^-20) every pixel deposits into node 0.
 *   3. C0, C1 = inclusive integer prefix sums of the source and target histograms, totals T0, T1.  For node k: the smallest
 *      j with C1[j] T0 >= C0[k] T1, compared as exact 128-bit products (exact for any counts the entry points admit);
 *      u' = 0 if j == 0, else j - 1 + (C0[k] T1 - C1[j-1] T0) / (C1[j] T0 - C1[j-1] T0), the two differences converted to
 *      fp64 and divided there.  M[k] = lo1 + u' / (n - 1) (hi1 - lo1) in fp64, stored as fp32.  Flat stretches of the target
 *      CDF map to their left end.
 *   4. v' = (1 - t) M[k] + t M[k + 1] with the k, t of step 2, d_a = v' - v.
 *   5. If !(hi0 - lo0 > 2^-20), d_a = 0 (no division happens).  A degenerate target axis needs no case: every M[k] = lo1.
 * Then x_j += rho R_i^T d_j.  After the last rotation the output is clipped to [0, 1] and written as (n_src, 3) HWC, fp32
 * (16-byte aligned) or uint8 = (uint8)(v * 255) (truncation, 4-byte aligned) when out_u8 != 0, as hg_color_affine.
 * Histograms, prefix sums and the search are integers, so nothing depends on the order of a sum: repeats are bit-identical.
 *
 * Device state, in the caller's workspace slots (hg_idt_run lays them out in its own workspace):
 *   a range set   uint32[6] = enc(lo[0..2]), enc(hi[0..2]) with enc(f) = bits(f) ^ 0xffffffff when f is negative, else
 *                 bits(f) | 0x80000000: unsigned order is float order, so min / max are integer atomics.  Cleared = (0xffffffff
 *                 x 3, 0 x 3).
 *   a histogram   uint64[3 * bins], axis-major.  Cleared = 0.
 *   a map         fp32[3 * bins], axis-major.
 *   the planes    the working copy of the source: fp32[3 * hg_idt_plane_stride(n)], channel c of pixel p at
 *                 [c * stride + p], stride = n rounded up to a multiple of 4, 16-byte aligned.
 * Limits: hg_idt_max_bins() nodes (3 * bins uint32 counters, and as many fp32 map nodes, in 48 KiB of LDS); pixel counts in
 * [1, 2^32 - 1]; a workgroup flushes its LDS counters after every hg_idt_block_pixels() (< 65536) pixels, so they cannot
 * overflow; hg_idt_target_chunk(bins) = the rotations whose counters fit LDS together, i.e. that one histogram launch takes;
 * hg_idt_blocks(n) = the workgroups every per-pixel launch gives n pixels (each a contiguous share, a multiple of 4 pixels,
 * walked hg_idt_group_pixels() = 256 lanes x 4 pixels at a time on the planes).
 * The queries return 0 for refused arguments.
 * Refusals, before any launch: a NULL or misaligned pointer, a non-positive stride HG_EINVAL; bins < 2 HG_EIDT_BINS;
 * bins > hg_idt_max_bins() HG_EIDT_BINS_LDS; iterations (nrot) < 1, or nrot > hg_idt_target_chunk(bins) in hg_idt_hist,
 * HG_EIDT_ITERATIONS; relaxation outside (0, 1] HG_EIDT_RELAXATION; a pixel count outside [1, 2^32 - 1] HG_EIDT_PIXELS; a
 * workspace below hg_idt_workspace_bytes HG_EWORKSPACE.
 *
 *   hg_idt_clear          resets n_ranges range sets and n_counters histogram counters (either may be 0).
 *   hg_idt_range          steps 1 of nrot rotations over strided pixels: atomic min / max into ranges[nrot][6] (cleared by the
 *                         caller); with planes != NULL also writes the working copy.
 *   hg_idt_hist           step 2 of nrot <= hg_idt_target_chunk(bins) rotations with the given range sets, added to
 *                         hist[nrot][3 * bins].  Pixels with pix_stride 1, a 16-byte aligned base and a chan_stride that is a
 *                         multiple of 4 and at least hg_idt_plane_stride(n) (the planes) are read 16 bytes per lane.  blocks: 0 =
 *                         hg_idt_blocks(n), else that many workgroups (at most 2048).
 *   hg_idt_table          step 3 from a source and a target histogram and the target's range set, one workgroup per axis;
 *                         then zeroes src_hist (clear_src_hist != 0) and clears the range set next_range (unless NULL).
 *   hg_idt_apply          steps 4, 5 and the update on the planes with the source's range set `range` and the map.  With
 *                         rotation_next != NULL the planes are updated in place and the range of the updated pixels'
 *                         projections with rotation_next is reduced into next_range (cleared before) in the same pass;
 *                         with rotation_next == NULL it is the last rotation: the clipped result goes to `out`.
 *   hg_idt_target_tables  range sets and histograms of the target for all rotations (clears them first): one pass for the
 *                         ranges, then one histogram launch per hg_idt_target_chunk(bins) rotations.
 *   hg_idt_run            the whole transfer, enqueued on `stream` with no host read-back: target tables, one range pass over
 *                         the source (which also makes the planes), then hist, table, apply per rotation (per rotation the
 *                         source is read twice and written once: 36 bytes per pixel). */
int hg_idt_block_pixels(void);
int hg_idt_max_bins(void);
int hg_idt_group_pixels(void);
int hg_idt_target_chunk(int32_t bins);
int hg_idt_blocks(int64_t n);
int64_t hg_idt_plane_stride(int64_t n);
size_t hg_idt_workspace_bytes(int64_t n_src, int64_t n_tgt, int32_t iterations, int32_t bins);
int hg_idt_clear(uint32_t *ranges, int64_t n_ranges, uint64_t *hist, int64_t n_counters, void *stream);
int hg_idt_range(const float *x, int64_t n, int64_t pix_stride, int64_t chan_stride, const float *rotations, int32_t nrot,
                 uint32_t *ranges, float *planes, void *stream);
int hg_idt_hist(const float *x, int64_t n, int64_t pix_stride, int64_t chan_stride, const float *rotations, int32_t nrot,
                int32_t bins, const uint32_t *ranges, uint64_t *hist, int32_t blocks, void *stream);
int hg_idt_table(uint64_t *src_hist, const uint64_t *tgt_hist, const uint32_t *tgt_range, int32_t bins, float *map,
                 uint32_t *next_range, int32_t clear_src_hist, void *stream);
int hg_idt_apply(float *planes, int64_t n, const float *rotation, const float *rotation_next, int32_t bins,
                 const uint32_t *range, const float *map, float relaxation, uint32_t *next_range, void *out, int32_t out_u8,
                 void *stream);
int hg_idt_target_tables(const float *target, int64_t n, int64_t pix_stride, int64_t chan_stride, const float *rotations,
                         int32_t iterations, int32_t bins, uint32_t *tgt_range, uint64_t *tgt_hist, void *stream);
int hg_idt_run(const float *source, int64_t n_src, int64_t src_pix_stride, int64_t src_chan_stride, const float *target,
               int64_t n_tgt, int64_t tgt_pix_stride, int64_t tgt_chan_stride, const float *rotations, int32_t iterations,
               int32_t bins, float relaxation, void *out, int32_t out_u8, void *workspace, size_t workspace_bytes,
               void *stream);

/* Palette extraction and palette-based colour transfer (since version 114; no code of the reference).  An image is described
 * by K colours, and a recolouring is carried to a photo by moving every pixel with a smooth blend of per-cluster shifts.
 * Everything that decides a palette is an integer, so nothing depends on the order of a sum and repeats are bit-identical.
 *
 * Points.  A pixel is four little-endian 16-bit integers (qL, qa, qb, qw), 8 bytes; a batch is int16 (B, stride, 4) with
 *   stride = hg_palette_point_stride(n) = n rounded up to a multiple of 2 (the kernels read two points, 16 bytes, per lane),
 *   16-byte aligned.  (L, a, b) = the chain of hg_srgb_to_lab above in fp64 on the fp32 input clamped to [0, 1], unrounded, in
 *   Lab units (hg_lab::srgb_to_lab_f64); q = rint(128 value), signed: inside the sRGB gamut |q| < 2^14, and a squared distance
 *   is dE76^2 in units of 1/128.  qw = rint(65535 clamp(w, 0, 1)), unsigned, 65535 without a weight map.  A pixel with a
 *   non-finite channel or weight has qw = 0 and coordinates 0, and so have the padding points between n and the stride.
 *   1 <= n <= 2^28 - 1 pixels per image, so that every signed 64-bit sum below stays under 2^59.
 * Bins.  16^3 cells: bL = min(max(qL, 0) / 800, 15), ba = clamp((qa + 16384) >> 11, 0, 15), bb likewise, cell = (bL 16 + ba) 16
 *   + bb.  A cell holds int64 (W, S_L, S_a, S_b) = sum qw, sum qw (qL, qa, qb) over its points with qw > 0: int64 (B, 4096, 4).
 *   Its mean is m = floor((2 S + W) / (2 W)) per component (floor division: nearest, halves up).
 * Seeds.  Weighted farthest-point selection over the cells, 1 <= K <= hg_palette_max_k() = 16, one workgroup per image, on the
 *   device.  Seed 0 = the mean of the cell of largest W, the lowest cell index on ties.  Seed j = the mean of the cell that
 *   maximises W_i min_{l<j} d^2(m_i, seed_l), the products compared exactly (128 bits), the lowest cell index on ties.  When
 *   the maximum is 0 the remaining seeds are copies of seed 0; without any weight every seed is (0, 0, 0).
 * Centres.  int32 (B, K, 3), coordinates within 16 bits.  Distances d^2 are exact integers (64 bits).
 * Lloyd step.  Two point sets of one length, `assign` and `value` (the same pointer for k-means), and K centres.  Every point
 *   of `assign` with qw > 0 goes to the centre of least d^2, the lowest index on ties; cluster k receives W_k += qw and
 *   S_k += qw (the coordinates of the point of `value` at the same position; its qw is not read): int64 sums (B, K, 4) =
 *   (W, S_L, S_a, S_b), ADDED to what the caller left there.  Optionally a uint8 label per pixel, (B, n), 255 where qw = 0.
 *   With a second image as `value` the sums give the paired palette: the mean of that image over each cluster's pixels.
 *   A workgroup adds into 64-bit LDS counters (no bound on its share is needed: the totals stay under 2^59) and flushes
 *   them to the global ones with 64-bit integer atomics.  There are no float atomics.
 * Update.  c_k = floor((2 S_k + W_k) / (2 W_k)) per component; a cluster with W_k = 0 keeps its centre.
 * Run.  quantise, bins, seeds, `iterations` >= 0 times (step, update), then one last step that leaves W, S and the labels of the
 *   final centres.  A fixed iteration count, no convergence read-back: everything is enqueued on `stream`.  With `other` !=
 *   NULL (a second image of the same size, its own strides) the run ends with a step whose `value` is that image and an
 *   update into centres_other, which starts as a copy of the centres, and with an update of the centres from the sums of the
 *   last step: both palettes are then means over the same clusters (those of the labels), t_k - s_k is the mean shift of
 *   cluster k, an image paired with itself gives centres_other == centres, and so does an empty cluster.
 * Transfer.  Source centres s_k and destination centres t_k, fp32 (K, 3) in Lab units, int32 live[K], on the device.  Per pixel
 *   x = Lab(clamp(rgb, 0, 1)) in fp64 (a NaN component reads as 0); over the live k, in index order:
 *     d_k = |x - s_k|^2, u_k = exp(-(d_k - min_l d_l) / (2 sigma^2)), y = x + sum_k u_k (t_k - s_k) / sum_k u_k
 *   and y = x without a live centre.  The output is y through the inverse chain (fp64), clipped to [0, 1], rounded once: (n, 3)
 *   HWC fp32 (16-byte aligned), or uint8 = (uint8)(v * 255) (truncation, 4-byte aligned) when out_u8 != 0, as hg_color_affine.
 *   sigma > 0 is used as given; sigma <= 0 asks for the default, computed on the device in fp64 in a fixed order: the mean of
 *   |s_i - s_j| over the live pairs i < j, and 1 when there is no pair or the mean is 0.  Either way the value used is written
 *   to sigma_used (one device float), which the per-pixel kernel reads: no host synchronisation between an extraction and a
 *   transfer.  Pixels are addressed as in hg_color_moments.
 * Plan.  hg_palette_blocks(n) = the workgroups a per-point launch gives an image of n points (each a contiguous share, a
 *   multiple of 2 points; grid = blocks x B); `blocks` = 0 takes the plan, 1 .. 1024 forces that count -- the result has the
 *   same bits.  hg_palette_workspace_bytes(B, n, paired): the points (of both images when paired != 0), the cells and the paired
 *   sums of hg_palette_run; 16-byte aligned.  The queries return 0 for refused arguments.
 * Refusals, before any launch: a NULL or misaligned pointer, B outside [1, 65535], a size < 1, blocks outside [0, 1024],
 *   iterations < 0, only one of other and centres_other, a non-positive stride or a non-finite sigma in the transfer: HG_EINVAL;
 *   K outside [1, 16]: HG_EPALETTE_K; n (or H W) outside [1, 2^28 - 1]: HG_EPALETTE_PIXELS; a workspace below
 *   hg_palette_workspace_bytes: HG_EWORKSPACE.
 * hg_palette_quantize takes x as fp32 (B, 3, H, W) and the optional weight as fp32 (B, H, W), each with its own element strides
 * (as hg_delta_e); hg_palette_bins adds into `bins` (the caller clears them); hg_palette_update zeroes the sums it has read
 * when clear_sums != 0. */
#define HG_PALETTE_MAX_K 16
int hg_palette_max_k(void);
int hg_palette_blocks(int64_t n);
int64_t hg_palette_point_stride(int64_t n);
size_t hg_palette_workspace_bytes(int32_t B, int64_t n, int32_t paired);
int hg_palette_quantize(const float *x, int64_t xs_b, int64_t xs_c, int64_t xs_h, int64_t xs_w, const float *weight, int64_t ws_b,
                        int64_t ws_h, int64_t ws_w, int16_t *points, int32_t B, int32_t H, int32_t W, void *stream);
int hg_palette_bins(const int16_t *points, int32_t B, int64_t n, int64_t *bins, int32_t blocks, void *stream);
int hg_palette_seeds(const int64_t *bins, int32_t B, int32_t K, int32_t *centres, void *stream);
int hg_palette_step(const int16_t *assign, const int16_t *value, int32_t B, int64_t n, const int32_t *centres, int32_t K,
                    int64_t *sums, uint8_t *labels, int32_t blocks, void *stream);
int hg_palette_update(int64_t *sums, int32_t B, int32_t K, int32_t *centres, int32_t clear_sums, void *stream);
int hg_palette_run(const float *x, int64_t xs_b, int64_t xs_c, int64_t xs_h, int64_t xs_w, const float *weight, int64_t ws_b,
                   int64_t ws_h, int64_t ws_w, const float *other, int64_t os_b, int64_t os_c, int64_t os_h, int64_t os_w,
                   int32_t B, int32_t H, int32_t W, int32_t K, int32_t iterations, int32_t blocks, int32_t *centres,
                   int64_t *sums, int32_t *centres_other, uint8_t *labels, void *workspace, size_t workspace_bytes,
                   void *stream);
int hg_palette_transfer(const float *x, int64_t n, int64_t pix_stride, int64_t chan_stride, const float *src_centres,
                        const float *dst_centres, const int32_t *live, int32_t K, float sigma, float *sigma_used, void *out,
                        int32_t out_u8, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HG_POST_H */
