"""Is a change to the host side of hg_conv.hip invisible from outside?  Three dumps of the tree this file lies in, each run
once in a checkout of the parent and once in the change and compared (profiles/conv_route_identity.json and
profiles/conv_route_bench.json record which of them were run, and what they showed).  Only entry points that the parent has
are called, so the same file runs in both trees (it needs tests/test_conv_route_gpu.py beside it for `gpu`):

  python tools/conv_route_check.py host  OUT.json    no GPU: hg_conv2d_plan (return code and the five ints),
                                                     hg_conv2d_workspace_bytes for dgrad 0 and 1 and
                                                     hg_conv2d_wgrad_workspace_bytes over a grid of arguments, as one sha256
                                                     per (ksize, stride, H) block plus counts
  python tools/conv_route_check.py gpu   OUT.json    the case list of tests/test_conv_route_gpu.py and the bench layer shapes
                                                     at batch 2: each case's HG_CONV_DEBUG stderr lines and a
                                                     sha256 of every output, data gradient and weight gradient
  python tools/conv_route_check.py calls OUT.json [OTHER.so]
                                                     host cost: wall time to issue one forward + data-gradient + weight-gradient
                                                     C-ABI triple at a shape where the kernels take microseconds; with the other
                                                     tree's library as OTHER.so both are timed alternately in ONE process

`host` and `gpu` outputs of two trees are equal when the files are (`cmp`); run `gpu` twice in one tree first to learn which
cases repeat bit for bit (all should: the kernels sum in fixed order)."""
import ctypes
import hashlib
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

BS = (1, 2, 7, 32, 64)
CH = (1, 3, 16, 17, 32, 33, 64, 65, 128, 512, 2048)
HS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 64, 256)
STRIDES = (1, 2, 3)          # 3: invalid


def host(out_path):
    from histogan_amd._lib import lib
    plan = (ctypes.c_int32 * 5)()
    blocks, codes, calls = {}, {}, 0
    for ksize, stride, H in itertools.product((1, 3), STRIDES, HS):
        hsh = hashlib.sha256()
        for W, B, K, N in itertools.product((H, 1, H + 1), BS, CH, CH):
            for dgrad in (0, 1):
                for i in range(5):
                    plan[i] = -1
                rc = lib.hg_conv2d_plan(B, K, N, H, W, ksize, stride, dgrad, plan)
                hsh.update(repr((rc, tuple(plan), lib.hg_conv2d_workspace_bytes(B, K, N, H, W, ksize, stride, dgrad))).encode())
                codes[str(rc)] = codes.get(str(rc), 0) + 1
            hsh.update(repr(lib.hg_conv2d_wgrad_workspace_bytes(B, K, N, H, W, ksize, stride)).encode())
            calls += 5
        blocks['ksize=%d stride=%d H=%d' % (ksize, stride, H)] = hsh.hexdigest()
    json.dump({'calls': calls, 'argument_sets': calls // 5, 'hg_conv2d_plan return codes': codes, 'sha256_per_block': blocks},
              open(out_path, 'w'), indent=1, sort_keys=True)
    print('host:', calls, 'calls,', len(blocks), 'blocks')


def gpu_cases():
    """(name, case) in the form tests/test_conv_route_gpu.py run_case takes: its own list, then the generator's 3x3 layers and
    the discriminator's stride-2 / 1x1 shapes of the benchmark (256 px, capacity 16) at batch 2."""
    import test_conv_route_gpu as T
    cases = [(T.case_id(c), c) for c in T.CASES]
    f = [64] + [16 * 2 ** (i + 1) for i in range(7)][::-1]          # bench.py g_layers(256, 16)
    for i in range(7):
        S = 4 * 2 ** i
        shapes = [(K, N, S, 3, 1, fe) for K, N in ((f[i], f[i + 1]), (f[i + 1], f[i + 1])) for fe in (False, True)]
        shapes += [(f[i + 1], 3, S, 1, 1, True), (f[i + 1], f[i + 1], 2 * S, 3, 2, False)]      # to-RGB, the discriminator's down-sampling
        for K, N, H, k, stride, fe in shapes:
            for op in ('fwd', 'dgrad', 'wgrad'):
                if not (fe and op == 'wgrad'):
                    c = T.Case(2, K, N, H, H, k, stride, fe, op)
                    cases.append(('bench ' + T.case_id(c), c))
    return cases


def gpu(out_path):
    os.environ['HG_CONV_DEBUG'] = '1'             # read once by the library, at its first launch
    import tempfile
    import torch
    import test_conv_route_gpu as T
    dev = torch.device('cuda:0')
    sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    res = {}
    for i, (name, case) in enumerate(gpu_cases()):
        # the launch lines are written to the C stderr (unbuffered): file descriptor 2 points at a file for the case
        with tempfile.TemporaryFile() as tmp:
            sys.stderr.flush()
            saved = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            try:
                out = T.run_case(case, dev)
                torch.cuda.synchronize()
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            tmp.seek(0)
            lines = tmp.read().decode().splitlines()
        res['%03d %s' % (i, name)] = {'launches': [ln for ln in lines if ln.startswith('k_conv')], 'sha256': {k: sha(v) for k, v in out.items()}}
    json.dump(res, open(out_path, 'w'), indent=1, sort_keys=True)
    print('gpu:', len(res), 'cases,', sum(len(v['launches']) for v in res.values()), 'launch lines')


def calls(out_path, other_lib=None):
    """other_lib: a second libhistogan_hip.so (the other tree's) loaded into the same process; the repetitions then alternate
    between the two libraries, so both see the same process, clocks and allocator state."""
    import torch
    from histogan_amd._lib import check, lib
    libs = {'this': lib}
    if other_lib:
        libs['other'] = ctypes.CDLL(other_lib)
        for fn in ('hg_conv_packed_elems', 'hg_conv_pack_weights_both', 'hg_conv2d_workspace_bytes', 'hg_conv2d_wgrad_workspace_bytes',
                   'hg_conv2d_fwd', 'hg_conv2d_dgrad', 'hg_conv2d_wgrad'):
            getattr(libs['other'], fn).argtypes, getattr(libs['other'], fn).restype = getattr(lib, fn).argtypes, getattr(lib, fn).restype
    dev = torch.device('cuda:0')
    res = {}
    for name, (B, K, N, H, k, stride) in (('3x3 2x16->16 16x16', (2, 16, 16, 16, 3, 1)), ('3x3 stride 2 2x16->16 16x16', (2, 16, 16, 16, 3, 2)),
                                          ('1x1 2x16->3 16x16', (2, 16, 3, 16, 1, 1)), ('3x3 K split 2x512->512 4x4', (2, 512, 512, 4, 3, 1))):
        Ho = (H - 1) // stride + 1
        x, go = torch.randn(B, K, H, H, device=dev), torch.randn(B, N, Ho, Ho, device=dev)
        w = torch.randn(N, K, k, k, device=dev)
        wf = torch.empty(lib.hg_conv_packed_elems(N, K, k, 0), device=dev)
        wd = torch.empty(lib.hg_conv_packed_elems(N, K, k, 1), device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        check(lib.hg_conv_pack_weights_both(w.data_ptr(), wf.data_ptr(), wd.data_ptr(), N, K, k, st), 'pack')
        y, gx, gw = torch.empty(B, N, Ho, Ho, device=dev), torch.empty_like(x), torch.empty_like(w)
        nf, nd = lib.hg_conv2d_workspace_bytes(B, K, N, H, H, k, stride, 0), lib.hg_conv2d_workspace_bytes(B, N, K, H, H, k, stride, 1)
        nw = lib.hg_conv2d_wgrad_workspace_bytes(B, K, N, H, H, k, stride)
        ws = torch.empty(max(nf, nd, nw, 4), dtype=torch.uint8, device=dev)
        a_f = (x.data_ptr(), wf.data_ptr(), y.data_ptr(), None, None, None, B, K, N, H, H, k, stride, ws.data_ptr(), nf, st)
        a_d = (go.data_ptr(), wd.data_ptr(), gx.data_ptr(), None, None, B, N, K, H, H, k, stride, ws.data_ptr(), nd, st)
        a_w = (x.data_ptr(), go.data_ptr(), gw.data_ptr(), None, None, B, K, N, H, H, k, stride, ws.data_ptr(), ws.numel(), st)
        reps = {t: [] for t in libs}
        for rep in range(6 if not other_lib else 11):                      # the first repetition is the warm-up
            for t, l in libs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(2000):
                    check(l.hg_conv2d_fwd(*a_f), 'fwd')
                    check(l.hg_conv2d_dgrad(*a_d), 'dgrad')
                    check(l.hg_conv2d_wgrad(*a_w), 'wgrad')
                t_issue = time.perf_counter() - t0
                torch.cuda.synchronize()
                reps[t].append({'issue_us_per_triple': t_issue / 2000 * 1e6, 'done_us_per_triple': (time.perf_counter() - t0) / 2000 * 1e6})
        res[name] = reps['this'][1:] if not other_lib else {t: v[1:] for t, v in reps.items()}
    json.dump(res, open(out_path, 'w'), indent=1, sort_keys=True)
    med = lambda v: sorted(r['issue_us_per_triple'] for r in v)[len(v) // 2]
    print('calls:', {k: med(v) if not other_lib else {t: med(r) for t, r in v.items()} for k, v in res.items()})


if __name__ == '__main__':
    {'host': host, 'gpu': gpu, 'calls': calls}[sys.argv[1]](*sys.argv[2:4])
