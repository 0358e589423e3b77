/* hg_hist.h -- C ABI of the MI355X-native RGB-uv histogram (libhistogan_hip.so).
 *
 * Drop-in boundary for histogram_classes/RGBuvHistBlock.py:75-228 of the
 * reference (RGBuvHistBlock.forward) and for the autograd replay of that chain
 * (SURVEY.md section 8a, rows a2-a7).  The reference has no native code; these
 * entry points are what a ctypes binding inside RGBuvHistBlock.forward calls
 * (see INTEGRATION.md).
 *
 * Conventions: every function returns 0 on success, a negative HG_E* code on an
 * argument error, or a positive hipError_t.  Functions never allocate, free or
 * synchronise; all device work is enqueued on `stream` (a hipStream_t passed as
 * void*; NULL = the legacy default stream).  All pointers except the params
 * struct are DEVICE pointers.  fp32 everywhere.  Re-entrant.
 */
#ifndef HG_HIST_H
#define HG_HIST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HG_OK 0
#define HG_EINVAL (-1)    /* bad argument (NULL pointer, non-positive size, ...)        */
#define HG_EMETHOD (-2)   /* unknown kernel method  (RGBuvHistBlock.py:141-144)          */
#define HG_ERESIZE (-3)   /* unknown resize mode    (RGBuvHistBlock.py:90-93)            */
#define HG_EWORKSPACE (-4)/* workspace too small                                         */
#define HG_EUNSUPPORTED (-5)
/* the refusals of the distribution transfer (hg_idt_*, hg_post.h), one code each */
#define HG_EIDT_BINS (-20)        /* bins < 2                                             */
#define HG_EIDT_BINS_LDS (-21)    /* bins > hg_idt_max_bins(): the counters exceed LDS    */
#define HG_EIDT_ITERATIONS (-22)  /* iterations < 1, or more rotations than one call takes */
#define HG_EIDT_RELAXATION (-23)  /* relaxation outside (0, 1]                            */
#define HG_EIDT_PIXELS (-24)      /* a pixel count outside [1, 2^32 - 1]                  */
/* the refusals of the palette (hg_palette_*, hg_post.h) */
#define HG_EPALETTE_K (-25)      /* palette: K outside [1, hg_palette_max_k()]           */
#define HG_EPALETTE_PIXELS (-26)  /* palette: a pixel count outside [1, 2^28 - 1]         */
/* the refusals of the 3D LUTs (hg_lut_*, hg_lut.h) */
#define HG_ELUT_SIZE (-27)        /* LUT: N outside [2, hg_lut_max_n()]                   */
#define HG_ELUT_PIXELS (-28)      /* LUT fit: more than hg_lut_max_pixels() pixel pairs   */
/* the refusals of regrain (hg_regrain_*, hg_regrain.h) */
#define HG_EREGRAIN_SIZE (-29)        /* regrain: H or W below 2, or more than 2^28 pixels */
#define HG_EREGRAIN_ITERATIONS (-30)  /* regrain: no level, or a level with fewer than 1 sweep */
#define HG_EREGRAIN_SMOOTHNESS (-31)  /* regrain: smoothness not positive and finite        */
#define HG_EREGRAIN_MIN_SIDE (-32)    /* regrain: min_side below 1                          */

/* soft-bin kernel, RGBuvHistBlock.py:124-140 */
#define HG_METHOD_THRESHOLDING 0
#define HG_METHOD_RBF 1
#define HG_METHOD_INVERSE_QUADRATIC 2

#define HG_PROJ_RGBUV 0
#define HG_PROJ_RGCHROMA 1
#define HG_PROJ_DIRECT 2
#define HG_PROJ_LAB 3        /* since version 107 */

/* stage-0 resize, RGBuvHistBlock.py:77-95 */
#define HG_RESIZE_NONE 0      /* H<=insz and W<=insz: pixels used as they are            */
#define HG_RESIZE_BILINEAR 1  /* F.interpolate(size=(Hs,Ws), bilinear, align_corners=False) */
#define HG_RESIZE_SAMPLING 2  /* x.index_select(2,row_idx).index_select(3,col_idx)        */

typedef struct hg_hist_params {
  /* sizeof(hg_hist_params) as the CALLER compiled it (ABI guard, since version 102): every entry point returns
   * HG_EINVAL when it differs from the library's, so a caller built against an older header -- or one that did not
   * zero the struct and fill this in -- is rejected instead of having trailing fields (proj_cache: a pointer the
   * forward WRITES through) read as garbage. */
  uint32_t struct_size;
  /* input image batch x: (B, C>=3, H, W), element strides (any layout) */
  int32_t B, C, H, W;
  int64_t stride_b, stride_c, stride_h, stride_w;
  /* pixels entering the histogram: Hs x Ws (== H x W for HG_RESIZE_NONE) */
  int32_t Hs, Ws;
  int32_t resize_mode;
  const int32_t *row_idx; /* device, Hs entries, HG_RESIZE_SAMPLING only */
  const int32_t *col_idx; /* device, Ws entries, HG_RESIZE_SAMPLING only */
  /* histogram definition (ctor args of RGBuvHistBlock, RGBuvHistBlock.py:29-73) */
  int32_t h;              /* bins per axis                                               */
  double lo, hi;          /* sorted hist_boundary                                        */
  int32_t method;         /* HG_METHOD_*                                                 */
  double sigma;           /* RBF / inverse-quadratic width (ignored for thresholding)    */
  int32_t intensity_scale;
  int32_t green_only;     /* only plane 1 (log g/r, log g/b), written at plane index 0   */
  /* 2-D projection of a pixel (HG_PROJ_*).  0: RGB-uv log-chroma, 3 planes.  The two one-plane variants of the
   * reference's other histogram blocks share everything else (clamp, resize, kernels, normalisation):
   * 1: rg-chroma (u,v) = (R,G)/(R+G+B+1e-6), weight Iy   (histogram_classes/rgChromaHistBlock.py:100-141)
   * 2: direct     (u,v) = channels (1,2), weight = channel 0  (histogram_classes/LabHistBlock.py:102-140)
   * 3: Lab        the input is sRGB; the clamped / resized pixel is converted to normalised CIE Lab (Ln, an, bn) =
   *               (L/100, (a+128)/255, (b+128)/255) -- sRGB transfer curve, the D65 matrix of hg_srgb_to_lab (hg_post.h)
   *               with every row divided by its sum, f(t) = cbrt(t) above (6/29)^3 and t/(3 (6/29)^2) + 4/29 below --
   *               evaluated in fp64 and rounded ONCE to fp32; from there on it is a `direct` pixel: (u,v) = (an, bn),
   *               weight = Ln.  The backward goes through the 3x3 Jacobian of that chain at the pixel.  Routes,
   *               workspaces and cache use are those of 2. */
  int32_t projection;
  /* 1: the F.relu the train step puts in front of the block (histoGAN/histoGAN.py:955) is part of the call -- identical
   * forward (clamp(relu(x)) == clamp(x)); the backward masks x <= 0 instead of x < 0.  Saves that aten launch and node. */
  int32_t pre_relu;
  /* Optional device buffer of B * Hs * Ws * 32 bytes (16-byte aligned), or NULL.  The forward stores every pixel's
   * projection (log-chroma differences, Iy, clamped / resized colour, the resized `weight` value) there; a backward call given the SAME
   * buffer reads it instead of re-sampling and re-projecting (bilinear taps + three fp64 logarithms per pixel).
   * Smooth kernels (inverse-quadratic, dense RBF) only; the scatter paths ignore it. */
  void *proj_cache;
  /* Optional per-pixel weight map (since version 103), or NULL = every pixel counts fully (the strides are then not
   * read).  Device, fp32, one value per INPUT pixel: element (b, y, x) at weight[b*weight_stride_b + y*weight_stride_h
   * + x*weight_stride_w], element strides, any layout; a stride of 0 broadcasts the map over that axis (one map for the
   * whole batch: weight_stride_b = 0).  Values are taken as clamp(w, 0, 1).  Stage 0 resizes the map exactly like a
   * colour channel (same bilinear taps / same row_idx, col_idx gather); histogram pixel n then enters with the weight
   * w_n * Iy_n (w_n * 1 without intensity_scale, w_n * channel 0 for HG_PROJ_DIRECT, w_n * Ln for HG_PROJ_LAB).  grad_x is the gradient with w fixed
   * (exactly 0 where w_n == 0); hg_rgbuv_hist_bwd treats the map as a constant, hg_rgbuv_hist_bwd_w (since version 105)
   * also produces its gradient.  Either backward call must be given the same map as the forward.  Every kernel path
   * honours it. */
  const float *weight;
  int64_t weight_stride_b, weight_stride_h, weight_stride_w;
} hg_hist_params;

/* library / build identification */
int hg_version(void);
const char *hg_error_string(int code);

/* Self-test of the scatter path's fast window classification (method = thresholding): exhaustive error of the
 * hardware logarithm it uses over every float in [1e-6, 1 + 2e-6], against the fp64 logarithm rounded to fp32 that
 * the exact path (and the reference's CPU logf, RGBuvHistBlock.py:112-114) evaluates.  out2 (device, 2 floats):
 * [0] = max relative error where |ln x| >= 1e-3, [1] = max absolute error elsewhere.  The classification's margins
 * assume [0] <= 3e-7 and [1] <= 3e-7 (hg_hist.hip: kFastLogRel, kFastAbs carry the roundings on top). */
int hg_selftest_fastlog(float *out2, void *stream);

/* 1 when a forward / backward pair with these params uses `proj_cache` (the dense MFMA kernels), 0 when it would be
 * ignored (thresholding, the truncated-RBF scatter / gather pair): lets the caller skip the 32 B / pixel allocation.
 * Negative HG_E* on bad params. */
int hg_rgbuv_hist_uses_proj_cache(const hg_hist_params *p);

/* Which kernel families a call with these params runs on (since version 106).  The library decides this once per call;
 * the same decision sizes the workspaces and picks the launches, and this query returns it.  DESIGN.md section 4 has the
 * table of conditions. */
enum {
  HG_ROUTE_FWD_DENSE = 0,       /* k_hist_fwd (MFMA, split-K over pixels) -> k_hist_finish                          */
  HG_ROUTE_FWD_THR_SCATTER = 1, /* k_hist_thr_fwd -> k_hist_finish                                                  */
  HG_ROUTE_FWD_THR_LEAN = 2,    /* k_thr_fwd_lean [-> k_hist_finish when fwd_slices > 1]                            */
  HG_ROUTE_FWD_RBF_SCATTER = 3  /* k_hist_rbf_fwd (truncated at rbf_radius bins) -> k_hist_finish                   */
};
enum {
  HG_ROUTE_BWD_MIRRORED = 0,    /* k_hist_bwd (MFMA, mirrored-bin merge)                                            */
  HG_ROUTE_BWD_PLANES = 1,      /* k_hist_bwd_planes<planes_rt> (MFMA, one plane at a time)                         */
  HG_ROUTE_BWD_GENERIC = 2,     /* k_hist_ghat -> k_hist_bwd_generic                                                */
  HG_ROUTE_BWD_THR_GATHER = 3,  /* k_hist_ghat -> k_hist_thr_bwd                                                    */
  HG_ROUTE_BWD_RBF_GATHER = 4,  /* k_hist_ghat -> k_hist_rbf_bwd                                                    */
  HG_ROUTE_BWD_THR_LEAN = 5,    /* k_thr_bwd_lean                                                                   */
  HG_ROUTE_BWD_ZERO = 6         /* no kernel: grad_x is cleared (the gradient is identically zero)                  */
};                              /* every backward is followed by the resize adjoint when resize_mode != NONE        */

typedef struct hg_hist_route {
  int32_t struct_size;          /* in: sizeof(hg_hist_route) as the caller compiled it (ABI guard, like the params) */
  int32_t fwd, bwd;             /* HG_ROUTE_FWD_*, HG_ROUTE_BWD_*                                                    */
  int32_t fwd_slices;           /* split-K slices per image of the forward                                          */
  int32_t bwd_workgroups;       /* workgroups per image of the backward kernel `bwd` names (0 for ZERO)             */
  int32_t planes_rt;            /* PLANES: 32-bin row tiles, ceil(h / 32); else 0                                    */
  int32_t rbf_radius;           /* RBF_SCATTER / RBF_GATHER: support radius in bins; else 0                          */
  int32_t uses_proj_cache;      /* == (fwd == HG_ROUTE_FWD_DENSE), what hg_rgbuv_hist_uses_proj_cache returns        */
} hg_hist_route;

/* Fills *out (all fields but struct_size) for a forward / backward pair with these params.  weight_grad != 0: the
 * backward is hg_rgbuv_hist_bwd_w, and the params are validated like that call's (p->weight == NULL: HG_EINVAL; a
 * broadcast map: HG_EUNSUPPORTED); only `bwd` and `bwd_workgroups` can depend on it.  Launches nothing, touches no
 * device and needs none.  out == NULL or a stale out->struct_size: HG_EINVAL.  The environment switches HG_RBF_DENSE,
 * HG_THR_EXACT and HG_BWD_PLANES are read on every call, here as in the launching entry points. */
int hg_rgbuv_hist_route(const hg_hist_params *p, int weight_grad, hg_hist_route *out);

/* Bytes of scratch each call needs for these params (both may be queried at once). */
int hg_rgbuv_hist_workspace_bytes(const hg_hist_params *p, size_t *fwd_bytes, size_t *bwd_bytes);

/* Forward: hist_out (B, P, h, h) contiguous, P = green_only ? 1 : 3, L1-normalised per
 * image as RGBuvHistBlock.py:224-228;  sum_out (B) = sum of the raw histogram + 1e-6
 * (the normaliser, needed by the backward). */
int hg_rgbuv_hist_fwd(const hg_hist_params *p, const float *x, float *hist_out, float *sum_out,
                      void *workspace, size_t workspace_bytes, void *stream);

/* Backward: grad_x (B, C, H, W) contiguous, fully written (channels >= 3 get 0).
 * grad_out (B, P, h, h) contiguous; hist_out / sum_out as produced by the forward. */
int hg_rgbuv_hist_bwd(const hg_hist_params *p, const float *x, const float *grad_out,
                      const float *hist_out, const float *sum_out, float *grad_x,
                      void *workspace, size_t workspace_bytes, void *stream);

/* Backward with the gradient of the weight map (since version 105): hg_rgbuv_hist_bwd, same grad_x bit for bit, plus
 * grad_weight (B, H, W) contiguous, fully written: dL/dw at the INPUT resolution of the map -- per histogram pixel
 * m_n * sum_p k(u_p)^T Ghat_p k(v_p) with m_n the pixel's non-map factor (Iy, 1 without intensity_scale, channel 0 for
 * HG_PROJ_DIRECT, Ln for HG_PROJ_LAB), taken through the adjoint of the resize and masked by the map's clamp (passes where 0 <= w <= 1, both
 * ends inclusive; exactly 0 elsewhere).  Thresholding included (a gather of Ghat at the pixel's bins), also without
 * intensity_scale, where grad_x is identically zero.  p->weight == NULL or grad_weight == NULL: HG_EINVAL; a map with a
 * zero stride (broadcast): HG_EUNSUPPORTED -- expand it into memory first and reduce the gradient afterwards.
 * Workspace: hg_rgbuv_hist_bwd_w_workspace_bytes (the resized paths carry one more plane than hg_rgbuv_hist_bwd). */
int hg_rgbuv_hist_bwd_w_workspace_bytes(const hg_hist_params *p, size_t *bytes);
int hg_rgbuv_hist_bwd_w(const hg_hist_params *p, const float *x, const float *grad_out, const float *hist_out,
                        const float *sum_out, float *grad_x, float *grad_weight, void *workspace,
                        size_t workspace_bytes, void *stream);

/* Hellinger histogram loss, histoGAN/histoGAN.py:957-960:
 *   loss = alpha / sqrt(2) * sqrt( sum_{b,p,i,j} (sqrt(t) - sqrt(g))^2 ) / B
 * n = B*P*h*h elements.  loss_out (1); grad_gen (n) may be NULL (forward only).
 * grad_gen = d loss / d gen (not yet multiplied by an upstream gradient).
 * workspace: hg_hellinger_workspace_bytes(n). */
size_t hg_hellinger_workspace_bytes(int64_t n);
int hg_hellinger_fwd_bwd(const float *target, const float *gen, int64_t n, int32_t batch,
                         float alpha, float *loss_out, float *grad_gen, void *workspace,
                         size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HG_HIST_H */
