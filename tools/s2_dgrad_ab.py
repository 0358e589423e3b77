#!/usr/bin/env python3
"""Alternating timing of the stride-2 data gradients of the discriminator's down-sampling layers (the `D*.down ... dgrad` shapes
of tools/step_budget.py at B = 64 and B = 32, straight through hg_conv2d_dgrad): this tree's library and another tree's (the
parent's libhistogan_hip.so) loaded into ONE process, 5 alternating repetitions of 20 launches each after a warm-up one; also
whether the two results are bit-equal.  profiles/s2_dgrad_allclass.json `kernel_level` is its output.

    python tools/s2_dgrad_ab.py OUT.json OTHER.so"""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from histogan_amd._lib import check, lib
other = ctypes.CDLL(os.path.abspath(sys.argv[2]))
for fn in ('hg_conv2d_dgrad',):
    getattr(other, fn).argtypes, getattr(other, fn).restype = getattr(lib, fn).argtypes, getattr(lib, fn).restype
libs = {'parent': other, 'change': lib}
dev = torch.device('cuda:0')
st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
REPS, ITERS = 5, 20
res = {}
for B in (64, 32):
    for i in range(7):
        C, S = 16 * 2 ** i, 256 // 2 ** i
        So = S // 2
        go = torch.randn(B, C, So, So, device=dev)
        w = torch.randn(C, C, 3, 3, device=dev) / (C * 9) ** 0.5
        wd = torch.empty(lib.hg_conv_packed_elems(C, C, 3, 1), device=dev)
        check(lib.hg_conv_pack_weights(w.data_ptr(), wd.data_ptr(), C, C, 3, 1, st), 'pack')
        nd = lib.hg_conv2d_workspace_bytes(B, C, C, S, S, 3, 2, 1)
        ws = torch.empty(max(nd, 8), dtype=torch.uint8, device=dev)
        gx = {t: torch.full((B, C, S, S), float('nan'), device=dev) for t in libs}
        times = {t: [] for t in libs}
        for rep in range(REPS + 1):
            for t, l in libs.items():
                args = (go.data_ptr(), wd.data_ptr(), gx[t].data_ptr(), None, None, B, C, C, S, S, 3, 2, ws.data_ptr(), nd, st)
                check(l.hg_conv2d_dgrad(*args), 'dgrad')
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(ITERS):
                    l.hg_conv2d_dgrad(*args)
                e1.record()
                torch.cuda.synchronize()
                if rep: times[t].append(e0.elapsed_time(e1) / ITERS * 1e3)   # us
        same = bool(torch.equal(gx['parent'], gx['change']))
        byts = (go.numel() + gx['change'].numel()) * 4
        med = {t: sorted(v)[len(v) // 2] for t, v in times.items()}
        res['B%d D%d.down %d->%d @%d' % (B, i, C, C, S)] = dict(us=times, median_us=med, bit_equal=same, finite=bool(torch.isfinite(gx['change']).all()),
            tbps={t: byts / med[t] / 1e6 for t in libs}, tflops={t: 2.0 * B * So * So * C * C * 9 / med[t] / 1e6 for t in libs})
        print('B%d D%d: parent %.1f us  change %.1f us  (min %.1f / %.1f)  equal %s  TB/s %.2f -> %.2f' % (B, i, med['parent'], med['change'],
              min(times['parent']), min(times['change']), same, byts / med['parent'] / 1e6, byts / med['change'] / 1e6), flush=True)
json.dump(res, open(sys.argv[1], 'w'), indent=1, sort_keys=True)
