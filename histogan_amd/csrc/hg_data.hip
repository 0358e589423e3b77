// hg_data.hip -- the device-resident image source (include/hg_data.h): Pillow's uint8 bilinear resample, one axis per launch
// for a batch of differently sized items, and the ToTensor / flip finish.  Byte gathers bound by memory latency: one thread
// per output byte (per output float in the finish), 3 to 9 taps re-read through L1/L2, no LDS staging.  Rows are 3 W bytes
// at any alignment and images lie back to back, so nothing wider than a byte is loaded or stored on the uint8 side.
#include "hg_host.h"
#include "../../include/hg_data.h"

namespace {

// grid (ceil(max_bytes / 256), items); a block past its item's extent exits
template <int AXIS>
__global__ __launch_bounds__(256) void k_data_resample(const hg_data_item *__restrict__ items,
                                                       const int *__restrict__ bounds, const int *__restrict__ coeffs,
                                                       int n_tab, int ksize) {
  const hg_data_item it = items[blockIdx.y];
  const unsigned per = AXIS == 1 ? 3u * (unsigned)it.n_out : (unsigned)it.n_keep;   // bytes of one output row
  const unsigned long long total = (unsigned long long)per * (unsigned)(AXIS == 1 ? it.n_keep : it.n_out);
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  if (it.n_out <= 0 || it.n_keep <= 0 || idx >= total) return;
  const unsigned row = idx / per, col = idx - row * per;
  const unsigned o = AXIS == 1 ? col / 3u : row;              // position along the resampled axis
  const long long tr = (long long)it.tab_off + o;
  if (tr < 0 || tr >= n_tab) return;
  const int first = bounds[2 * tr] - it.in_base;
  int count = bounds[2 * tr + 1];
  count = count < ksize ? count : ksize;
  const int *k = coeffs + tr * ksize;
  const uint8_t *src = reinterpret_cast<const uint8_t *>(it.src);
  // tap t reads src[base + t * step]
  const long long step = AXIS == 1 ? 3 : it.src_stride;
  const long long base = AXIS == 1 ? (long long)row * it.src_stride + (col - 3u * o) + 3LL * first
                                   : (long long)first * it.src_stride + col;
  int acc = 1 << 21;
  for (int t = 0; t < count; ++t) {
    const int p = first + t;
    if (p < 0 || p >= it.in_len) continue;
    acc += k[t] * (int)src[base + t * step];
  }
  acc >>= 22;
  acc = acc < 0 ? 0 : (acc > 255 ? 255 : acc);
  reinterpret_cast<uint8_t *>(it.dst)[(long long)row * it.dst_stride + col] = (uint8_t)acc;
}

// grid (ceil(3 S S / 256), items)
__global__ __launch_bounds__(256) void k_data_finish(const hg_data_item *__restrict__ items, int S, float *__restrict__ out) {
  const unsigned plane = (unsigned)S * S, idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= 3u * plane) return;
  const hg_data_item it = items[blockIdx.y];
  const unsigned c = idx / plane, rem = idx - c * plane, y = rem / S, x = rem - y * S;
  const unsigned xs = (it.flags & 1) ? S - 1 - x : x;
  const uint8_t v = reinterpret_cast<const uint8_t *>(it.src)[(long long)y * it.src_stride + 3 * xs + c];
  out[(size_t)blockIdx.y * 3 * plane + idx] = (float)v / 255.f;   // a division, as k_u8_hwc_to_f32: ToTensor's bits
}

}  // namespace

extern "C" {

int hg_data_max_ksize(void) { return HG_DATA_MAX_KSIZE; }
int hg_data_item_bytes(void) { return (int)sizeof(hg_data_item); }

int hg_data_resample_axis(const hg_data_item *items, int32_t n_items, int32_t axis, int64_t max_bytes, const int32_t *bounds,
                          const int32_t *coeffs, int32_t n_tab, int32_t ksize, void *stream) {
  if (!items || !bounds || !coeffs || n_items <= 0 || n_tab <= 0 || ksize < 1 || ksize > HG_DATA_MAX_KSIZE ||
      (axis != 0 && axis != 1) || max_bytes < 1 || max_bytes > 0x7fffffffLL)
    return HG_EINVAL;
  const long long nb = (max_bytes + 255) / 256;
  if (!grid_ok(nb, n_items, 1)) return HG_EINVAL;
  const dim3 grid((unsigned)nb, (unsigned)n_items);
  return dispatch([&](auto AXIS) {
    return launch(k_data_resample<AXIS>, grid, dim3(256), 0, (hipStream_t)stream, items, bounds, coeffs, n_tab, ksize);
  }, among<0, 1>(axis));
}

int hg_data_finish(const hg_data_item *items, int32_t n_items, int32_t S, float *out, void *stream) {
  if (!items || !out || n_items <= 0 || S < 1 || S > 16384) return HG_EINVAL;
  const long long nb = (3LL * S * S + 255) / 256;
  if (!grid_ok(nb, n_items, 1)) return HG_EINVAL;
  return launch(k_data_finish, dim3((unsigned)nb, (unsigned)n_items), dim3(256), 0, (hipStream_t)stream, items, S, out);
}

}  // extern "C"
