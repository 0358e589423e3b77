/* hg_wino.h -- C ABI of the Winograd F(2x2, 3x3) form of the 3x3 stride-1 convolutions (libhistogan_hip.so).
 *
 * The contraction inside Conv2DMod.forward (histoGAN/histoGAN.py:431-439), the 3x3 convolutions of
 * DiscriminatorBlock.net (:510-515) and their data gradients are 3x3, stride 1, zero padding 1.  For those the
 * minimal-filtering form  Y = A^T [ (G g G^T) . (B^T d B) ] A  needs 16 multiplications per 2x2 output tile and input
 * channel instead of 36: the sixteen transform positions are sixteen independent (N x K) x (K x tiles) contractions on
 * v_mfma_f32_32x32x2_f32 -- still exact fp32 products with fp32 accumulation, 2.25x fewer of them.  Measured against
 * fp64 the result is CLOSER than the direct fma chain (sixteen chains of depth K instead of one of depth 9 K; transforms
 * are additions and halvings only): 4e-7 ... 1.6e-6 max-norm relative where the direct kernel sits at 1.1e-6 ... 3.0e-6.
 *
 * Conventions as hg_conv.h: 0 / negative HG_E* / positive hipError_t; device pointers; the caller's stream; nothing is
 * allocated or synchronised.  HG_EUNSUPPORTED = this shape is not served (odd H / W, K % 8, too few tiles): the caller
 * uses hg_conv2d_fwd / hg_conv2d_dgrad.
 */
#ifndef HG_WINO_H
#define HG_WINO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when hg_wino_conv2d serves (B, K, N, H, W) -- K input channels, N output channels of the launch (for a data
 * gradient K = the convolution's output channels) -- AND is expected to beat the direct kernel there. */
int hg_wino_supported(int32_t B, int32_t K, int32_t N, int32_t H, int32_t W);

/* Transformed-weight operand U = G g G^T in the kernel's lane order.  mode as hg_conv_pack_weights (HG_CONV_PACK_FWD:
 * K = Ci, N = Co; HG_CONV_PACK_DGRAD: K = Co, N = Ci, taps flipped).  Returns floats (0: weight shape not served). */
size_t hg_wino_packed_elems(int32_t Co, int32_t Ci, int32_t mode);
int hg_wino_pack_weights(const float *w, float *u, int32_t Co, int32_t Ci, int32_t mode, void *stream);

/* Every 3x3 weight of a model in ONE launch (after an optimizer step), as hg_conv_pack_weights_multi: `items_dev` =
 * device array of n_items descriptors; u_fwd / u_dgrad (hg_wino_packed_elems floats each) may be NULL (that operand is
 * not written); block_begin = running sum of hg_wino_pack_blocks(Co, Ci, u_fwd != NULL, u_dgrad != NULL) over the
 * preceding items, total_blocks = the sum over all. */
typedef struct hg_wino_pack_item {
  const float *w;
  float *u_fwd, *u_dgrad;
  /* optional (NULL: none; needs u_fwd): wsq[co][ci] = sum_taps W[co][ci][t]^2, as hg_pack_item.wsq of hg_conv.h (the weight
   * factor of the demodulation coefficient) -- so that a weight whose direct operands nobody asks for needs no direct pack */
  float *wsq;
  int32_t Co, Ci, block_begin, reserved;
} hg_wino_pack_item;
int32_t hg_wino_pack_blocks(int32_t Co, int32_t Ci, int32_t want_fwd, int32_t want_dgrad);
int hg_wino_pack_weights_multi(const hg_wino_pack_item *items_dev, int32_t n_items, int32_t total_blocks, void *stream);

/* Scratch of hg_wino_conv2d for these arguments (K-split slabs of launches that cannot fill the chip with output
 * tiles); 0 = none. */
size_t hg_wino_workspace_bytes(int32_t B, int32_t K, int32_t N, int32_t H, int32_t W);

/* out[b,n,y,x] = lrelu_slope( oscale[b,n] * sum_{k,dy,dx} iscale[b,k] in[b,k,y+dy-1,x+dx-1] W[n,k,dy,dx]
 *                             + bias[n] + noise_w[n] * noise_img[b,y,x] ) + addend[b,n,y,x]
 * (same epilogue as hg_modconv2d_fwd / hg_conv2d_fwd_add; every optional pointer may be NULL, lrelu_slope 0 = none,
 * addend only without scales / noise / activation); u from hg_wino_pack_weights. */
int hg_wino_conv2d(const float *in, const float *u, float *out, const float *iscale, const float *oscale,
                   const float *bias, const float *noise_w, const float *noise_img, int32_t noise_S, float lrelu_slope,
                   const float *addend, int32_t B, int32_t K, int32_t N, int32_t H, int32_t W, void *workspace,
                   size_t workspace_bytes, void *stream);

/* Weight gradient of that convolution on the same transform:  gw = G^T [ sum_tiles (A gout A^T) . (B^T in B) ] G
 *   in (B,K,H,W), gout (B,N,H,W), gw (N,K,3,3) contiguous, fully written; deterministic (per-split slabs in the
 *   workspace, summed in fixed order).  Maps whose sides are 2 x a power of two.  hg_wino_wgrad_supported: served AND
 *   expected to beat hg_conv2d_wgrad (>= 64 channels on both sides, maps >= 4x4). */
int hg_wino_wgrad_supported(int32_t B, int32_t K, int32_t N, int32_t H, int32_t W);
size_t hg_wino_wgrad_workspace_bytes(int32_t B, int32_t K, int32_t N, int32_t H, int32_t W);
int hg_wino_wgrad(const float *in, const float *gout, float *gw, int32_t B, int32_t K, int32_t N, int32_t H, int32_t W,
                  void *workspace, size_t workspace_bytes, void *stream);

/* Which launches hg_wino_conv2d / hg_wino_wgrad take (since version 112).  The library decides this once per call, as one
 * plan: the same plan sizes the workspace, answers the *_supported queries, fills the kernel arguments of the launches and
 * is what the two queries below return.  Host logic only: nothing is launched, no device is touched and none is needed
 * (256 CUs are assumed where no device answers).  The HG_WINO_* environment knobs act on the plan, so the route reports
 * what they force. */
typedef struct hg_wino_query {
  int32_t struct_size;          /* sizeof(hg_wino_query) as the caller compiled it (ABI guard)                               */
  int32_t B, K, N, H, W;        /* as passed to hg_wino_conv2d / hg_wino_wgrad                                               */
  int32_t fe;                   /* hg_wino_conv2d: != 0: the call passes iscale (the kernel instance with the input scale)  */
  int32_t have_workspace;       /* the call's workspace != NULL                                                              */
  size_t workspace_bytes;       /* the call's workspace_bytes ((size_t)-1: as the workspace query plans, "unlimited")        */
} hg_wino_query;

typedef struct hg_wino_plan {
  int32_t struct_size;          /* in: sizeof(hg_wino_plan) as the caller compiled it (ABI guard)                           */
  int32_t variant;              /* 0: k_wino<2,2,8> (64 channels x 64 tiles, 8-channel chunks), 1: k_wino<1,4,4> (32 x 128, 4) */
  int32_t fe;                   /* the FE instance of that kernel (input scale)                                              */
  int32_t nblk, nch;            /* channel blocks of N, K chunks                                                             */
  int32_t lTW, lTH, lNI;        /* log2 of a block's tile grid: tiles per row, rows, images                                  */
  int32_t bt_x, bt_y;           /* block tiles per map row / column (ragged where tiles_w, tiles_h are no multiple)          */
  int32_t blocks;               /* work items per K split: nblk x bt_x x bt_y x image groups                                 */
  int32_t ksplit;               /* K splits as launched (1: the kernel writes `out` itself)                                  */
  int32_t chunks_per_split;     /* ceil(nch / ksplit): split z owns chunks [z, z + 1) x that, clamped to nch                 */
  int32_t last_split_chunks;    /* chunks of the last split that owns any (1 ... chunks_per_split)                           */
  int32_t empty_splits;         /* trailing splits that own no chunk (they store zero slabs)                                 */
  int32_t xcd;                  /* 1: the channel blocks of a block tile are dispatched eight apart (one XCD)                */
  int32_t grid;                 /* workgroups launched: min(blocks x ksplit, CUs) (HG_WINO_PERSIST=0: blocks x ksplit)       */
  int32_t persistent;           /* 1: blocks x ksplit > grid -- workgroups loop over work items                              */
  int32_t reduce;               /* 1: k_wino_reduce follows (ksplit > 1)                                                     */
  int32_t cus;                  /* compute units planned for                                                                 */
  int32_t supported;            /* == hg_wino_supported(B, K, N, H, W)                                                       */
  int32_t reserved;
  size_t slab_bytes;            /* workspace the route uses: ksplit x B x N x H x W x 4 (== hg_wino_workspace_bytes for an
                                   unlimited workspace), 0 without a split                                                   */
} hg_wino_plan;

typedef struct hg_wino_wgrad_plan {
  int32_t struct_size;          /* in: sizeof(hg_wino_wgrad_plan) as the caller compiled it (ABI guard)                     */
  int32_t lPW, lPH, lPI;        /* log2 of the 8-tile chunk pattern: tiles per row, rows, images                             */
  int32_t lcg, lrg;             /* log2 of the column / row groups of a map                                                  */
  int32_t nchunks;              /* chunks of the launch: image groups x row groups x column groups                           */
  int32_t ktiles, ntiles;       /* 64-channel tiles of K and N                                                               */
  int32_t splits;               /* pixel splits (slabs)                                                                      */
  int32_t chunks_per_split;     /* ceil(nchunks / splits)                                                                    */
  int32_t last_split_chunks;    /* chunks of the last split that owns any                                                    */
  int32_t empty_splits;         /* trailing splits that own no chunk (they store zero slabs)                                 */
  int32_t reduce_groups;        /* SG of k_wino_wgrad_reduce<SG>: 32 (splits >= 16), 8 (>= 4) or 1                           */
  int32_t xcd;                  /* 1: the (n, k) tiles of a split are dispatched eight apart (one XCD)                       */
  int32_t grid;                 /* workgroups launched: min(ktiles x ntiles x splits, CUs)                                   */
  int32_t persistent;           /* 1: more blocks than workgroups                                                            */
  int32_t cus;                  /* compute units planned for                                                                 */
  int32_t supported;            /* == hg_wino_wgrad_supported(B, K, N, H, W)                                                 */
  int32_t reserved;
  size_t slab_bytes;            /* == hg_wino_wgrad_workspace_bytes(B, K, N, H, W)                                           */
} hg_wino_wgrad_plan;

/* Fill *out (all fields but struct_size) for the call `q` describes.  Return codes are those of the call: NULL pointers
 * or a stale struct_size HG_EINVAL, a shape the call does not serve HG_EUNSUPPORTED; hg_wino_wgrad_route also HG_EINVAL
 * without a workspace and HG_EWORKSPACE for one that is too small (hg_wino_wgrad refuses both), after filling *out. */
int hg_wino_route(const hg_wino_query *q, hg_wino_plan *out);
int hg_wino_wgrad_route(const hg_wino_query *q, hg_wino_wgrad_plan *out);

#ifdef __cplusplus
}
#endif
#endif /* HG_WINO_H */
