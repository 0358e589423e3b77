"""Is a change to the host side of hg_hist.hip invisible from outside?  Three dumps of the tree this file lies in, each run
once in a checkout of the parent and once in the change and compared (profiles/hist_route_identity.json and
profiles/hist_route_bench.json record which of them were run, and what they showed):

  python tools/hist_route_check.py host  OUT.json    no GPU: workspace sizes, projection-cache answers and return codes of
                                                     the C ABI over a grid of params and the three environment switches,
                                                     as one sha256 per (switch state, h) block plus counts
  python tools/hist_route_check.py gpu   OUT.json    sha256 of hist, grad_x and grad_weight for the case lists of the
                                                     weighted-histogram GPU tests at their own shapes: without a map,
                                                     with a constant map, with weight_grad
  python tools/hist_route_check.py calls OUT.json    host cost: wall time per forward + backward C-ABI call pair at a
                                                     shape where the kernels take a few microseconds

`host` and `gpu` outputs of two trees are equal when the files are (`cmp`); run `gpu` twice in one tree first to learn
which cases repeat bit for bit (the sampling adjoint's float atomics need not)."""
import ctypes
import hashlib
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

H_LIST = (1, 2, 16, 32, 33, 40, 64, 65, 79, 80, 81, 96, 128, 129, 136, 140, 141, 142)
SWITCHES = [{}] + [{k: v} for k, vs in (('HG_RBF_DENSE', '01'), ('HG_THR_EXACT', '01'), ('HG_BWD_PLANES', '012')) for v in vs]
NAMES = ('HG_RBF_DENSE', 'HG_THR_EXACT', 'HG_BWD_PLANES')


def host(out_path):
    from histogan_amd import _lib as L
    lib, ref = L.lib, ctypes.byref
    p = L.HgHistParams()
    p.struct_size = ctypes.sizeof(L.HgHistParams)
    p.C, p.stride_w = 3, 1
    f, b, n = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    blocks, calls, codes = {}, 0, {}
    grid = list(itertools.product((0, 1, 2), (0.02, 0.05, 0.5), ((-3.0, 3.0), (-3.0, 1.0), (0.5, 3.0)), (0, 1, 2), (0, 1), (0, 1),
                                  (0, 1, 2), (1, 2, 32), ((16, 16), (40, 48), (41, 45), (150, 150), (256, 256)), (0, 1)))
    for sw in SWITCHES:
        for k in NAMES:
            os.environ.pop(k, None)
        os.environ.update(sw)
        for h in H_LIST:
            hsh = hashlib.sha256()
            p.h = h
            for method, sigma, (lo, hi), proj, green, intensity, resize, B, (Hs, Ws), wmap in grid:
                if method == 0 and sigma != 0.02:            # thresholding does not read sigma
                    continue
                H, W = (Hs, Ws) if resize == 0 else (2 * Hs, 2 * Ws)
                p.method, p.sigma, p.lo, p.hi, p.projection, p.green_only, p.intensity_scale = method, sigma, lo, hi, proj, green, intensity
                p.resize_mode, p.B, p.H, p.W, p.Hs, p.Ws = resize, B, H, W, Hs, Ws
                p.stride_b, p.stride_c, p.stride_h = 3 * H * W, H * W, W
                p.row_idx = p.col_idx = 0x1000 if resize == 2 else None
                p.weight = 0x2000 if wmap else None
                p.weight_stride_b, p.weight_stride_h, p.weight_stride_w = H * W, W, 1
                f.value = b.value = n.value = 0
                r = (lib.hg_rgbuv_hist_workspace_bytes(ref(p), ref(f), ref(b)), f.value, b.value,
                     lib.hg_rgbuv_hist_bwd_w_workspace_bytes(ref(p), ref(n)), n.value, lib.hg_rgbuv_hist_uses_proj_cache(ref(p)))
                hsh.update(repr(r).encode())
                calls += 3
                codes[str((r[0], r[3], r[5]))] = codes.get(str((r[0], r[3], r[5])), 0) + 1
            blocks['%s h=%d' % (','.join(f'{k}={v}' for k, v in sw.items()) or 'unset', h)] = hsh.hexdigest()
    for k in NAMES:
        os.environ.pop(k, None)
    json.dump({'calls': calls, 'param_sets': calls // 3, 'return_codes (workspace, bwd_w workspace, uses_proj_cache)': codes,
               'sha256_per_block': blocks}, open(out_path, 'w'), indent=1, sort_keys=True)
    print('host:', calls, 'calls,', len(blocks), 'blocks')


def gpu_cases():
    import test_hist_weight_cpu as C
    import test_hist_weight_gpu as G
    import test_hist_weight_grad_gpu as WG
    cases = [(proj, kw, (1, 3, 40, 48), 'bhw', False) for proj, kw in C.PIN_CASES + G.GPU_PIN_EXTRA]
    cases += list(WG.CASES)
    cases += [(proj, kw, shape, 'bhw', False) for proj, kw, shape in G.EXACT_CASES]
    cases += [('rgbuv', dict(method=m, sigma=0.02, h=64, insz=150), (2, 3, 150, 150), 'bhw', False) for m in ('inverse-quadratic', 'thresholding')]
    return cases


def gpu(out_path):
    import test_hist_weight_cpu as C
    import test_hist_weight_grad_cpu as WC
    from hist_weight_ref import make_block, sample_image
    dev = torch.device('cuda:0')
    sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    res = {}
    for i, (proj, kw, shape, layout, pre_relu) in enumerate(gpu_cases()):
        g = torch.Generator().manual_seed(100 + i)
        x = sample_image(*shape, g).to(dev)
        w = WC.on_device(C.make_weight(layout, shape[0], shape[2], shape[3], g), layout, dev)
        blk = make_block(proj, dev, **kw)
        entry = {}
        for mode in ('no map', 'constant map', 'weight_grad'):
            xr = x.clone().requires_grad_(True)
            wr = w.clone().requires_grad_(True) if mode == 'weight_grad' else w
            kwargs = dict(pre_relu=True) if pre_relu else {}          # (only the RGB-uv block has the keyword)
            if mode != 'no map':
                kwargs.update(weight=wr, weight_grad=mode == 'weight_grad')
            out = blk(xr, **kwargs)
            go = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).to(dev)
            out.backward(go)
            entry[mode] = {'hist': sha(out), 'grad_x': sha(xr.grad)}
            if mode == 'weight_grad':
                entry[mode]['grad_weight'] = sha(wr.grad)
        torch.cuda.synchronize()
        res[f'{i:02d} {proj} {sorted(kw.items())} {shape} {layout} pre_relu={pre_relu}'] = entry
    json.dump(res, open(out_path, 'w'), indent=1, sort_keys=True)
    print('gpu:', len(res), 'cases')


def calls(out_path):
    from histogan_amd import hist as HH
    from histogan_amd._lib import check, lib
    dev = torch.device('cuda:0')
    res = {}
    for name, kw in (('dense h=16 2x3x16x16', dict(h=16, insz=32)), ('lean thresholding h=16 2x3x16x16', dict(h=16, insz=32, method='thresholding')),
                     ('dense h=64 2x3x16x16', dict(h=64, insz=32))):
        x = torch.rand(2, 3, 16, 16, device=dev)
        p, keep = HH._make_params(x, HH.HistConfig(**kw))
        fb, bb = HH._ws_bytes(p)
        out, sums, gx = torch.empty(2, 3, p.h, p.h, device=dev), torch.empty(2, device=dev), torch.empty_like(x)
        gout = torch.rand(2, 3, p.h, p.h, device=dev) - 0.5
        ws = torch.empty(max(fb, bb, 4), dtype=torch.uint8, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        args_f = (ctypes.byref(p), x.data_ptr(), out.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws.numel(), st)
        args_b = (ctypes.byref(p), x.data_ptr(), gout.data_ptr(), out.data_ptr(), sums.data_ptr(), gx.data_ptr(), ws.data_ptr(), ws.numel(), st)
        reps = []
        for rep in range(6):                      # the first repetition is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(2000):
                check(lib.hg_rgbuv_hist_fwd(*args_f), 'fwd')
                check(lib.hg_rgbuv_hist_bwd(*args_b), 'bwd')
            t_issue = time.perf_counter() - t0
            torch.cuda.synchronize()
            reps.append({'issue_us_per_pair': t_issue / 2000 * 1e6, 'done_us_per_pair': (time.perf_counter() - t0) / 2000 * 1e6})
        res[name] = reps[1:]
    json.dump(res, open(out_path, 'w'), indent=1, sort_keys=True)
    print('calls:', {k: min(r['issue_us_per_pair'] for r in v) for k, v in res.items()})


if __name__ == '__main__':
    {'host': host, 'gpu': gpu, 'calls': calls}[sys.argv[1]](sys.argv[2])
