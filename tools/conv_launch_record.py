"""Which launches does the host side of hg_conv.hip make?  Without a GPU: the file is compiled for the host only, with
hipLaunchKernelGGL replaced by a recorder, and a driver calls the C ABI (fake device pointers, never dereferenced on the host)
over a grid of arguments -- forward with and without fused extras and the residual addend, data gradient, weight gradient,
each with a full, a one-byte-short and no workspace, and the packing launches.  Every launch is written down as kernel
instantiation (the symbol behind the kernel handle), grid, block, dynamic LDS, stream and the kernel arguments (ConvArgs,
ConvArgs4 and WgradArgs field by field, geometry and tap offsets included), with the HG_CONV_DEBUG lines, the
hipFuncSetAttribute calls and every return code in between.

    python tools/conv_launch_record.py OUT.txt [TREE]      TREE: the checkout whose hg_conv.hip is recorded (default: this one)

Two trees make the same launches when the files are equal (`cmp`): the check to make BEFORE a changed host side goes near a
GPU, where a wrong grid or geometry writes out of bounds.  (No device is asked: 256 CUs, 3 blocks per CU by registers.)"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRE = r'''
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <cstdlib>
template <class T> void rec_one(const T &v) {
  unsigned long long h = 1469598103934665603ull;
  const unsigned char *p = (const unsigned char *)&v;
  for (size_t i = 0; i < sizeof(T); ++i) h = (h ^ p[i]) * 1099511628211ull;
  printf(" %zu:%llx", sizeof(T), h);
}
template <class... A> void rec_args(const A &...a) { (rec_one(a), ...); }
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, lds, st, ...)                                                                      \
  do {                                                                                                                   \
    dim3 g_ = (g), b_ = (b);                                                                                             \
    printf("LAUNCH %p grid %u %u %u block %u %u %u lds %zu st %p args", (void *)(k), g_.x, g_.y, g_.z, b_.x, b_.y, b_.z, (size_t)(lds), (void *)(st)); \
    rec_args(__VA_ARGS__);                                                                                               \
    printf("\n");                                                                                                        \
  } while (0)
#define hipFuncSetAttribute(k, a, v) (printf("ATTR %p %d\n", (void *)(k), (int)(v)), hipSuccess)
#define hipGetLastError() hipSuccess
#define hipOccupancyMaxActiveBlocksPerMultiprocessor(n, k, t, l) (*(n) = 3, hipSuccess)
#define fprintf(f, ...) printf(__VA_ARGS__)
'''

POST = r'''
namespace {
void rec_one(const Geom &g) {
  printf(" G[%d %d %d|%d %d %d %d|%a %a %a|%d %d %d|%d %d]", g.lTW, g.lTH, g.lNI, g.TWp, g.IMS, g.HALO, g.CHS, g.inv_TWp, g.inv_IMS, g.inv_HALO,
         g.tiles_x, g.tiles_y, g.groups, g.lo_y, g.lo_x);
}
void rec_one(const ConvArgs &a) {
  printf(" CA[%p %p %p %p %p %p %p|%d %d %d %d %d|%d %d %d %d %d %d|%d %d %d|", a.in, a.wt, a.out, a.iscale, a.oscale, a.bias, a.addend, a.B, a.K, a.N,
         a.Kp, a.Np, a.Hi, a.Wi, a.Ho, a.Wo, a.Hc, a.Wc, a.os, a.oy, a.ox);
  const int taps = a.ntx == 3 ? 9 : a.ntx * (a.wrow_dy ? 2 : 1);
  for (int t = 0; t < taps; ++t) printf("%d,", a.toff[t]);
  printf("|%d %d %d %d|%d %p|%p %p %d %a]", a.ntx, a.wrow0, a.wrow_dy, a.wrow_dx, a.ksplit, a.ksplit > 1 ? (void *)a.slab : nullptr, a.noise_w, a.noise_img, a.noise_S, a.slope);
  rec_one(a.g);
}
void rec_one(const ConvArgs4 &a) {
  printf(" C4[%d %d %d %d|%d]", a.tiles[0], a.tiles[1], a.tiles[2], a.tiles[3], a.xcd_map);
  for (int c = 0; c < 4; ++c) if (a.tiles[c]) rec_one(a.c[c]);
}
void rec_one(const WgradArgs &a) {
  printf(" WA[%p %p %p %p %p|%d %d %d %d %d %d %d %d %d|%d %d %d %d %d|%p]", a.in, a.gout, a.slab, a.iscale, a.gscale, a.B, a.K, a.N, a.Hi, a.Wi, a.Ho, a.Wo,
         a.Kp32, a.Np32, a.tiles_x, a.tiles_y, a.nchunks, a.splits, a.ktiles, a.gw);
}
}
#undef fprintf
int main(int argc, char **argv) {
  setvbuf(stdout, nullptr, _IOFBF, 1 << 20);
  const float *P = (const float *)0x1000;
  auto F = [&](int i) { return (float *)(0x100000ull * i); };
  const int Bs[] = {1, 2, 7, 32}, Cs[] = {1, 3, 16, 17, 33, 64, 65, 128, 136, 512, 2048}, Hs[] = {1, 2, 3, 4, 5, 8, 9, 16, 17, 21, 64, 129, 256};
  const int ks[3][2] = {{3, 1}, {1, 1}, {3, 2}};
  for (auto &kk : ks) for (int H : Hs) for (int wi = 0; wi < 3; ++wi) for (int B : Bs) for (int K : Cs) for (int N : Cs) {
    const int W = wi == 0 ? H : wi == 1 ? 1 : H + 1, k = kk[0], s = kk[1];
    if ((long long)B * (K > N ? K : N) * H * W >= (1LL << 28)) continue;
    printf("CASE %d %d %d %d %d %d %d\n", B, K, N, H, W, k, s);
    for (int dgrad = 0; dgrad < 2; ++dgrad) {
      const size_t nb = hg_conv2d_workspace_bytes(B, K, N, H, W, k, s, dgrad);
      for (int fe = 0; fe < 2; ++fe)
        for (int ws = 0; ws < 3; ++ws) {
          if (ws && !nb) continue;
          void *wp = ws == 2 ? nullptr : (void *)F(9);
          const size_t wb = ws == 0 ? nb : ws == 1 ? nb - 1 : 0;
          int rc;
          if (dgrad) rc = hg_conv2d_dgrad(F(1), F(2), F(3), fe ? F(4) : nullptr, fe ? F(5) : nullptr, B, K, N, H, W, k, s, wp, wb, (void *)0x77);
          else if (fe && s == 1) rc = hg_modconv2d_fwd(F(1), F(2), F(3), F(4), nullptr, F(6), F(7), F(8), 300, 0.2f, B, K, N, H, W, k, wp, wb, (void *)0x77);
          else if (fe) rc = hg_conv2d_fwd(F(1), F(2), F(3), nullptr, F(5), F(6), B, K, N, H, W, k, s, wp, wb, (void *)0x77);
          else if (wi == 1) rc = hg_conv2d_fwd_add(F(1), F(2), F(3), F(10), F(6), B, K, N, H, W, k, s, wp, wb, (void *)0x77);
          else rc = hg_conv2d_fwd(F(1), F(2), F(3), nullptr, nullptr, F(6), B, K, N, H, W, k, s, wp, wb, (void *)0x77);
          printf("RC dgrad %d fe %d ws %d: %d\n", dgrad, fe, ws, rc);
        }
    }
    const size_t nw = hg_conv2d_wgrad_workspace_bytes(B, K, N, H, W, k, s);
    for (int sc = 0; sc < 2; ++sc)
      printf("RC wgrad %d: %d\n", sc, hg_conv2d_wgrad(F(1), F(2), F(3), sc ? F(4) : nullptr, sc ? F(5) : nullptr, B, K, N, H, W, k, s, F(9), nw, (void *)0x77));
    printf("RC wgrad short: %d\n", hg_conv2d_wgrad(F(1), F(2), F(3), nullptr, nullptr, B, K, N, H, W, k, s, F(9), nw - 1, (void *)0x77));
  }
  const int cc[][2] = {{16, 3}, {130, 70}, {1, 1}, {2048, 512}};
  for (auto &c : cc) for (int k : {1, 3}) {
    for (int m = 0; m < 3; ++m) printf("RC pack %d\n", hg_conv_pack_weights(F(1), F(2), c[0], c[1], k, m, (void *)0x77));
    printf("RC both %d\n", hg_conv_pack_weights_both(F(1), F(2), F(3), c[0], c[1], k, (void *)0x77));
  }
  printf("RC multi %d %d\n", hg_conv_pack_weights_multi((const hg_pack_item *)F(1), 5, 77, (void *)0x77), hg_conv_pack_weights_multi(nullptr, 5, 77, nullptr));
  printf("RC huge %d %d %d\n", hg_conv2d_fwd(F(1), F(2), F(3), nullptr, nullptr, nullptr, 64, 2048, 16, 256, 256, 3, 1, nullptr, 0, nullptr),
         hg_conv2d_dgrad(F(1), F(2), F(3), nullptr, nullptr, 1, 1 << 21, 136, 10, 10, 3, 2, nullptr, 0, nullptr),
         hg_conv2d_dgrad(F(1), F(2), F(3), nullptr, nullptr, 1, 1 << 21, 136, 10, 10, 3, 2, F(9), 1 << 30, nullptr));
  return 0;
}
'''


def main(out, tree=ROOT):
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'rec.hip'), os.path.join(d, 'rec')
        with open(src, 'w') as f:
            f.write(PRE + '#include "%s"\n' % os.path.join(tree, 'histogan_amd', 'csrc', 'hg_conv.hip') + POST)
        # host only: the device image the module constructor would register stays unresolved (nothing is launched)
        subprocess.check_call(['hipcc', '--offload-arch=gfx950', '-O1', '-std=c++17', '-no-pie', '--cuda-host-only', '-Wno-unused-value',
                               '-I', os.path.join(tree, 'include'), '-Wl,--unresolved-symbols=ignore-all', src, '-o', exe])
        names = {}
        for ln in subprocess.run(['nm', '-C', exe], capture_output=True, text=True, check=True).stdout.splitlines():
            p = ln.split(' ', 2)
            if len(p) == 3 and p[1] not in 'Uw':
                names['0x' + p[0].lstrip('0')] = p[2].replace('__device_stub__', '')
        run = subprocess.Popen([exe], stdout=subprocess.PIPE, text=True, env={'HG_CONV_DEBUG': '1'})
        hsh, lines, launches, kernels = hashlib.sha256(), 0, 0, set()
        with open(out, 'w') as f:
            for ln in run.stdout:
                m = re.match(r'(LAUNCH|ATTR) (0x[0-9a-f]+)', ln)
                if m:
                    kernels.add(names[m.group(2)])
                    ln = ln.replace(m.group(2), names[m.group(2)], 1)
                    launches += m.group(1) == 'LAUNCH'
                hsh.update(ln.encode())
                lines += 1
                f.write(ln)
        assert run.wait() == 0
    print('%d lines, %d launches of %d kernel instantiations, sha256 %s' % (lines, launches, len(kernels), hsh.hexdigest()))


if __name__ == '__main__':
    main(*sys.argv[1:3])
