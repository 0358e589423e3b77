// hg_host.h -- host-side helpers shared by the dispatchers (hg_hist.hip, hg_conv.hip, hg_wino.hip) and by the
// post-processing and metric launchers (hg_post.hip, hg_deltae.hip, hg_ssim.hip, hg_idt.hip): runtime values -> template
// arguments, the one kernel launch, the limits of a grid, and the per-device constants the planners read.
#pragma once
#include <type_traits>
#include "hg_common.h"
#include "../../include/hg_hist.h"   // HG_OK

namespace {

inline int ceil_log2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// what a launch accepts as its grid
inline bool grid_ok(long long gx, long long gy, long long gz) {
  return gx >= 1 && gx <= 0x7fffffffLL && gy >= 1 && gy <= 65535 && gz >= 1 && gz <= 65535;
}

// per-process caches are keyed by the CURRENT device (a process that launches on a second GPU must not plan with the first
// one's CU count, nor skip the dynamic-LDS attribute there): arrays of kMaxDev entries indexed by cur_dev()
constexpr int kMaxDev = 16;
inline int cur_dev() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) dev = 0;
  return dev;
}
inline int num_cus() {   // 256 where no device answers (the planners are host logic and run without one)
  static int n[kMaxDev] = {0};
  const int dev = cur_dev();
  if (!n[dev]) {
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, dev) == hipSuccess) n[dev] = pr.multiProcessorCount;
    if (n[dev] <= 0) n[dev] = 256;
  }
  return n[dev];
}

// ---- runtime values -> template arguments ---------------------------------------------------------------------------
// dispatch(f, picks...) calls the generic lambda f with one compile-time constant per pick: a bool becomes a
// std::bool_constant, among<V0, V1, ...>(v) the std::integral_constant<int, Vi> with Vi == v (the last one when none is).
template <int... Vs> struct Among { int v; };
template <int... Vs> Among<Vs...> among(int v) { return {v}; }

template <class F> int dispatch(F &&f) { return f(); }
template <class F, int V0, int... Vs, class... Rest> int dispatch(F &&f, Among<V0, Vs...> a, Rest... rest);

template <class F, class... Rest> int dispatch(F &&f, bool b, Rest... rest) {
  auto with = [&](auto c) { return dispatch([&](auto... cs) { return f(c, cs...); }, rest...); };
  return b ? with(std::true_type{}) : with(std::false_type{});
}

template <class F, int V0, int... Vs, class... Rest> int dispatch(F &&f, Among<V0, Vs...> a, Rest... rest) {
  auto head = [&] { return dispatch([&](auto... cs) { return f(std::integral_constant<int, V0>{}, cs...); }, rest...); };
  if constexpr (sizeof...(Vs) == 0) return head();
  else return a.v == V0 ? head() : dispatch(f, Among<Vs...>{a.v}, rest...);
}

// ---- the one launch ---------------------------------------------------------------------------------------------------
// launch + check, for a kernel whose dynamic LDS size the caller has already had allowed (hg_conv.hip fit_blocks_per_cu)
template <class... KArgs>
int launch_allowed(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t st, std::decay_t<KArgs>... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  HG_LAUNCH_CHECK();
  return HG_OK;
}
// dynamic LDS above 48 KB is asked for on the kernel that is launched
template <class... KArgs>
int launch(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t st, std::decay_t<KArgs>... args) {
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  return launch_allowed(kernel, grid, block, lds, st, args...);
}

}  // namespace
