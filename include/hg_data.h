/* hg_data.h -- C ABI of the device-resident image source (libhistogan_hip.so, since version 115): the uint8 transform of
 * the training Dataset -- Resize, CenterCrop or RandomResizedCrop, RandomHorizontalFlip, ToTensor -- on images that stay
 * on the device, for a whole batch in a constant number of launches.
 *
 *   hg_data_resample_axis     one axis of Pillow's uint8 bilinear resize (Image.resize(size, BILINEAR, box=...)), for a batch of
 *                             items of different sizes: uint8 HWC in, uint8 HWC out, 3 channels
 *   hg_data_finish            windowed uint8 HWC items -> one fp32 (B, 3, S, S) batch, v / 255 (torchvision ToTensor) with a
 *                             per-item horizontal flip
 *
 * Arithmetic.  Pillow's 8-bit resample is integer: the host turns the fp64 filter weights of an output position into
 * coefficients k[t] = (int)(0.5 + w[t] * 2^22) and the kernel computes
 *     out = clip((2^21 + sum_t k[t] * pix[first + t]) >> 22, 0, 255)
 * in int32 (the coefficients of a position sum to about 2^22, so 255 * 2^22 fits), over the `count` taps from `first` that the
 * bounds table names.  The tables are built by the host (histogan_amd.data.pil_bilinear_tables); the kernel accumulates and
 * shifts, so its bytes are Pillow's bytes.  A two-pass resize runs the horizontal axis first, over the source rows the vertical
 * pass reads, into a uint8 intermediate, then the vertical axis on that.
 *
 * Items.  A launch takes a device array of hg_data_item, one per image (grid.y = item); the items of a launch share the two
 * tables, each at its own row offset, and the tap stride `ksize` of the coefficient table (rows of an item with fewer taps are
 * zero-padded, and its bounds name fewer).  Rows are 3 W bytes at any byte alignment: every access is one byte.
 *
 * Conventions as in hg_hist.h: return 0 / negative HG_E* / positive hipError_t; device pointers; enqueue on `stream`; never
 * allocate or synchronise; nothing is launched for invalid arguments.  The item array is read by the kernel, not by the host:
 * the host-side figures a launch needs (the largest item) are arguments.
 */
#ifndef HG_DATA_H
#define HG_DATA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HG_DATA_MAX_KSIZE 256

/* One item of a launch (56 bytes, 8-byte aligned).
 *   hg_data_resample_axis, axis 1 (horizontal): for r < n_keep rows, o < n_out columns, c < 3
 *       dst[r * dst_stride + 3 o + c] = resample_t src[r * src_stride + 3 (first - in_base + t) + c]
 *   hg_data_resample_axis, axis 0 (vertical): for o < n_out rows, b < n_keep bytes of a row (3 x columns)
 *       dst[o * dst_stride + b] = resample_t src[(first - in_base + t) * src_stride + b]
 *   with (first, count) = bounds[tab_off + o] and the coefficients coeffs[(tab_off + o) * ksize + t].  An output window is the
 *   range [tab_off, tab_off + n_out) of an axis' table: what lies outside it is never computed.  in_base is the input
 *   index along the resampled axis that `src` points at (the first row of an intermediate that holds only the rows the
 *   vertical pass reads), in_len the number of input positions from there on: a tap outside [0, in_len) is not read.
 *   hg_data_finish reads src, src_stride and flags: out[item, c, y, x] = src[y * src_stride + 3 x' + c] / 255 with
 *   x' = S - 1 - x when flags & 1 (the flip follows the crop), x otherwise. */
typedef struct hg_data_item {
  uint64_t src;        /* device address */
  uint64_t dst;        /* device address (resample) */
  int64_t src_stride;  /* bytes between rows */
  int64_t dst_stride;
  int32_t n_out;
  int32_t n_keep;
  int32_t tab_off;
  int32_t in_base;
  int32_t in_len;
  int32_t flags;
} hg_data_item;

int hg_data_max_ksize(void);   /* HG_DATA_MAX_KSIZE */
int hg_data_item_bytes(void);  /* sizeof(hg_data_item): what a caller that lays the array out itself checks */

/* axis: 1 horizontal, 0 vertical.  bounds: int32 (n_tab, 2); coeffs: int32 (n_tab, ksize); a row past n_tab is not read.
 * max_bytes = the largest number of output bytes of one item (3 n_out n_keep for axis 1, n_out n_keep for axis 0): it sizes
 * grid.x, and tiles past an item's own extent exit.
 * HG_EINVAL: a NULL pointer, n_items outside [1, 65535], n_tab < 1, ksize outside [1, HG_DATA_MAX_KSIZE], an axis other
 * than 0 or 1, max_bytes outside [1, 2^31 - 1]. */
int hg_data_resample_axis(const hg_data_item *items, int32_t n_items, int32_t axis, int64_t max_bytes, const int32_t *bounds,
                          const int32_t *coeffs, int32_t n_tab, int32_t ksize, void *stream);

/* out: fp32 (n_items, 3, S, S), contiguous.  HG_EINVAL: a NULL pointer, n_items outside [1, 65535], S outside [1, 16384]. */
int hg_data_finish(const hg_data_item *items, int32_t n_items, int32_t S, float *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif
