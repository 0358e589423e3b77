"""Life of three registered 3x3 weights of one flat buffer over two optimizer steps (histogan_amd/wpack.py): what the batched
pack gives each of them follows from the launches that used it, and every launch computes what the per-call path computes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, K, N, H, W) of a 32 -> 32 channel layer on 128 x 128 maps: the Winograd kernel packs 128 tiles of 2 x 2 pixels into a
# block and is taken from half a block per CU on (hg_wino.hip: wino_beats_direct) -- 4 images are 128 blocks, the smallest
# batch that is served on 256 CUs; 3 images are 96 blocks, refused.
SERVED, REFUSED = (4, 32, 32, 128, 128), (3, 32, 32, 128, 128)


def test_registered_weights_follow_their_launches(gpu_device):
    from histogan_amd import conv as C
    from histogan_amd import wpack as W
    from histogan_amd._lib import lib
    from histogan_amd.optim import FlatParams
    assert lib.hg_wino_supported(*SERVED) == 1 and lib.hg_wino_supported(*REFUSED) == 0
    assert lib.hg_wino_packed_elems(32, 32, W.PACK_FWD) > 0 and lib.hg_wino_packed_elems(32, 32, W.PACK_DGRAD) > 0
    g = torch.Generator().manual_seed(5)
    a, b, c = ws = [torch.nn.Parameter((torch.randn(32, 32, 3, 3, generator=g) / 17).to(gpu_device)) for _ in range(3)]
    xs = torch.randn(SERVED[0], 32, 128, 128, generator=g).to(gpu_device)
    xr, x2 = xs[:REFUSED[0]].contiguous(), xs[:2, :, :16, :16].contiguous()
    # a: only where the Winograd kernel serves; b: only at stride 2; c: first where it refuses, then where it serves
    uses = [(a, xs, 1), (b, x2, 2), (c, xr, 1), (c, xs, 1)]
    flat = FlatParams(ws, with_grad=False)
    C.enable_pack_cache(ws)
    try:
        with torch.no_grad():
            for step in range(2):
                for w, x, stride in uses:
                    out = C.conv2d(x, w, None, stride)
                    assert torch.equal(out, C.conv2d(x, w.detach().clone(), None, stride)), (step, tuple(x.shape), stride)
                for w in ws:
                    wq = C.cached(w, 'wsq', lambda t: (_ for _ in ()).throw(AssertionError('wsq must come from the packing launch')))
                    assert torch.allclose(wq, w.detach().pow(2).sum(dim=(2, 3)), rtol=2e-6, atol=1e-7)
                ra, rb, rc = (W.record(w) for w in ws)
                if step == 1:       # the second pack: planned from what the first step's launches took
                    assert not ra.wants_direct and all(op.stale and op.winograd is not None for op in ra.ops)
                    assert rb.wants_direct and not rb.wants_wino and all(op.winograd is None and not op.stale for op in rb.ops)
                    assert rc.wants_direct and rc.wants_wino
                    assert rc.ops[W.PACK_FWD].winograd is not None and rc.ops[W.PACK_DGRAD].winograd is not None
                    assert not rc.ops[W.PACK_FWD].stale
                    assert [it.block is None for it in ra.owner.plan.sig] == [True, False, False]
                flat.data.mul_(1.25)
                C.weights_changed(flat.data)
    finally:
        C.enable_pack_cache(None)


def test_a_plan_outliving_its_weight_serves_the_successor_at_the_same_address(gpu_device):
    """Models come and go in one process and the allocator hands their addresses out again: the batched-pack plan of a flat
    buffer is found again by the successor (same owner, same weights, same decisions) and must pack from the LIVE weight."""
    import gc
    from histogan_amd import conv as C
    from histogan_amd import wpack as W
    g = torch.Generator().manual_seed(6)
    buf = torch.empty(32 * 32 * 9, device=gpu_device)
    x = torch.randn(2, 32, 16, 16, generator=g).to(gpu_device)
    try:
        with torch.no_grad():
            for generation in range(2):
                buf.copy_(torch.randn(buf.numel(), generator=g) / 17)
                w = torch.nn.Parameter(buf.view(32, 32, 3, 3))
                C.enable_pack_cache([w])
                rec = W.record(w)
                plan = rec.owner.plan
                assert (plan is None) == (generation == 0)
                out = C.conv2d(x, w, None, 2)        # stride 2: the direct operand, which the first plan of a weight leaves lazy
                assert (plan is None or rec.owner.plan is plan) and rec.ops[W.PACK_FWD].rec is rec
                assert torch.equal(out, C.conv2d(x, w.detach().clone(), None, 2))
                del w
                gc.collect()
    finally:
        C.enable_pack_cache(None)
