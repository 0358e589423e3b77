"""The generator differentiated with respect to its noise image, against frozen weights (projection):

1. hg_noise_grad (include/hg_nets.h) against the fp64 formula;
2. the per-block autograd nodes' gradient for nzt against fp64 autograd of the written-out stage;
3. the whole generator's noise gradient (one-node pass and per-block path) against oracle.histogan_nets in fp64 on the
   run's own LeakyReLU branches (the method of test_c3_parity_gpu.py's generator test);
4. the chain rule between forward_(inoise=) and forward_(noise1=, noise2=);
5. frozen weights: no weight-gradient launch, no flat-slot write, no AFTER_BLOCKS;
   and AFTER_BLOCKS only when no convolution / to-RGB weight gradient goes back to autograd (two passes before gather());
6. an in-place update of the noise image reaches the next forward (the cache of its transposed copy);
7. histogan_amd.project against the same Adam steps on the oracle.

Before this feature 3 and 5 fail with `noise.grad is None` / weight-gradient counters above zero (the fused backward
returned None for the noise and ignored needs_input_grad), 6 with a stale cached transpose, the others for want of
hg_noise_grad / histogan_amd.project."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import relmax
from oracle_step import LreluMasks

import noise_grad_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-5       # the bar tests/test_gstage_gpu.py holds the neighbouring sums to


def _np(t):
    return t.detach().cpu().numpy()


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------
KERNEL_CASES = [
    # B, O, H, S, demod
    (2, 8, 4, 16, True),          # a small window inside a larger noise image
    (1, 2048, 4, 4, True),        # channel-parallel reduction, H == S
    (3, 20, 8, 32, True),
    (2, 5, 32, 64, False),        # d = NULL
    (1, 3, 128, 128, True),
    (2, 6, 16, 16, True),
]


@pytest.mark.parametrize('B,O,H,S,demod', KERNEL_CASES)
def test_noise_grad_kernel_matches_fp64(B, O, H, S, demod, gpu_device):
    from histogan_amd.launch import noise_grad
    gconv, d, wn = R.noise_grad_inputs(B, O, H, demod, B * 1000 + O * 10 + H)
    want = R.noise_grad_fp64(gconv, d, wn)
    dev = gpu_device
    gc, dd, wv = gconv.to(dev), None if d is None else d.to(dev), wn.to(dev)
    # overwrite: a NaN-filled buffer gets a finite window and keeps its NaNs everywhere else
    buf = torch.full((B, S, S), float('nan'), device=dev)
    out = noise_grad(gc, dd, wv, buf, False)
    assert out is buf
    win = buf[:, :H, :H]
    assert bool(torch.isfinite(win).all())
    e = relmax(_np(win), want.numpy())
    print(f'noise_grad {B, O, H, S, demod}: overwrite relmax {e:.2e}')
    assert e <= TOL
    outside = torch.ones(B, S, S, dtype=torch.bool, device=dev)
    outside[:, :H, :H] = False
    assert bool(torch.isnan(buf[outside]).all())
    # bit-identical on a second launch
    buf2 = torch.zeros(B, S, S, device=dev)
    noise_grad(gc, dd, wv, buf2, False)
    assert torch.equal(buf2[:, :H, :H], win)
    # accumulate onto a random buffer: window = old + sum, everything else untouched bit for bit
    old = torch.randn(B, S, S, generator=torch.Generator().manual_seed(7)).to(dev)
    acc = old.clone()
    noise_grad(gc, dd, wv, acc, True)
    e = relmax(_np(acc[:, :H, :H]), (old[:, :H, :H].cpu().double() + want).numpy())
    print(f'noise_grad {B, O, H, S, demod}: accumulate relmax {e:.2e}')
    assert e <= TOL
    assert torch.equal(acc[outside], old[outside])
    acc2 = old.clone()
    noise_grad(gc, dd, wv, acc2, True)
    assert torch.equal(acc2, acc)


# ---- 2. the per-block nodes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,C,H,S', [(2, 8, 8, 16), (1, 4, 32, 32)])
@pytest.mark.parametrize('node', ['demod_noise_lrelu', 'conv_dnl', 'modconv_stage'])
def test_block_nodes_return_the_noise_gradient(node, B, C, H, S, gpu_device):
    from histogan_amd import ops
    dev = gpu_device
    g = torch.Generator().manual_seed(B * 100 + H)
    rnd = lambda *s: torch.randn(*s, generator=g)
    up = node == 'modconv_stage' and H == 32          # the up-sampled first convolution of a block at the larger shape
    x = rnd(B, C, H // 2, H // 2) if up else rnd(B, C, H, H)
    style, w = rnd(B, C) * 0.5, rnd(C, C, 3, 3) / (3 * C ** 0.5)
    wn, bn = rnd(C, 1) * 0.5, rnd(C) * 0.2
    nzt = torch.rand(B, S, S, generator=g)
    gout = rnd(B, C, H, H)
    nz = nzt.to(dev).requires_grad_(True)
    if node == 'demod_noise_lrelu':
        conv, d = rnd(B, C, H, H), torch.rand(B, C, generator=g) + 0.5
        out = ops.demod_noise_lrelu(conv.to(dev), d.to(dev), nz, wn.to(dev), bn.to(dev))
    elif node == 'conv_dnl':
        d = torch.rand(B, C, generator=g) + 0.5
        conv = F.conv2d(x.double(), w.double(), padding=1)
        out = ops.conv_dnl(x.to(dev), w.to(dev), d.to(dev), nz, wn.to(dev), bn.to(dev))
    else:
        conv, d = R.modconv_fp64(x, style, w, up), R.demod_fp64(style, w)
        out = ops.modconv_stage(x.to(dev), style.to(dev), w.to(dev), nz, wn.to(dev), bn.to(dev), demod=True, upsample=up)
    got, = torch.autograd.grad(out, nz, gout.to(dev))
    want = R.stage_nzt_grad_fp64(conv, d, nzt, wn.reshape(-1), bn, gout, out.detach().cpu() > 0)
    e = relmax(_np(got), want.numpy())
    print(f'{node} {B, C, H, S}: nzt gradient relmax {e:.2e}')
    assert got.shape == nzt.shape and e <= TOL
    if S > H:
        assert not bool(got[:, H:, :].any()) and not bool(got[:, :, H:].any())
    # not asked for: no gradient, and the other gradients are the same bits
    nz0 = nzt.to(dev)
    cd = conv.float().to(dev).requires_grad_(True) if node == 'demod_noise_lrelu' else x.to(dev).requires_grad_(True)
    for n_ in (nz, nz0):
        if node == 'demod_noise_lrelu':
            o = ops.demod_noise_lrelu(cd, d.to(dev), n_, wn.to(dev), bn.to(dev))
        elif node == 'conv_dnl':
            o = ops.conv_dnl(cd, w.to(dev), d.to(dev), n_, wn.to(dev), bn.to(dev))
        else:
            o = ops.modconv_stage(cd, style.to(dev), w.to(dev), n_, wn.to(dev), bn.to(dev), demod=True, upsample=up)
        gi, = torch.autograd.grad(o, cd, gout.to(dev))
        if n_ is nz:
            first = gi
    assert torch.equal(first, gi)


# ---- 3. the whole generator ------------------------------------------------------------------------------------------
def _generator(size, cap, seed, dev):
    from histogan_amd.nets import Generator
    torch.manual_seed(seed)
    G = Generator(size, 64, cap).to(dev)
    with torch.no_grad():
        for b in G.blocks:                      # (the reference initialises the noise projections to zero: make them count)
            for m in (b.to_noise1, b.to_noise2):
                m.weight.normal_(std=0.3)
                m.bias.normal_(std=0.1)
    return G


def _inputs(G, B, seed, dev):
    g = torch.Generator().manual_seed(seed)
    L, S = G.num_layers, G.image_size
    styles = torch.randn(B, L - 2, 64, generator=g).to(dev).requires_grad_(True)
    hists = torch.randn(B, 2, 64, generator=g).to(dev).requires_grad_(True)
    noise = torch.rand(B, S, S, 1, generator=g).to(dev)
    go = torch.randn(B, 3, S, S, generator=g).to(dev)
    return styles, hists, noise, go


def _run_recorded(G, styles, hists, noise, fused):
    """G(styles, hists, noise) with the LeakyReLU branches of its 2 L stages recorded, in forward order."""
    from histogan_amd import gfused, ops
    masks, orig_dnl, orig_cdnl = [], ops.demod_noise_lrelu, ops.conv_dnl

    def recording(orig):
        def f(*a):
            out = orig(*a)
            masks.append(out.detach().cpu() > 0)
            return out
        return f

    ops.demod_noise_lrelu, ops.conv_dnl = recording(orig_dnl), recording(orig_cdnl)
    gfused.STAGE_OBSERVER = lambda out: masks.append(out.detach().cpu() > 0)
    gfused.GFUSED = fused
    try:
        rgb = G(styles, hists, noise)
    finally:
        ops.demod_noise_lrelu, ops.conv_dnl = orig_dnl, orig_cdnl
        gfused.STAGE_OBSERVER = None
        gfused.GFUSED = True
    assert len(masks) == 2 * len(G.blocks)
    return rgb, masks


def _rms(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize('size,cap,B,seed', [(32, 2, 3, 3), (64, 4, 2, 21)])
def test_generator_noise_gradient_matches_fp64_oracle(size, cap, B, seed, gpu_device):
    from oracle import histogan_nets as N
    dev = gpu_device
    G = _generator(size, cap, seed, dev)
    styles, hists, noise, go = _inputs(G, B, seed, dev)
    L = G.num_layers

    def oracle(dt):
        sd = {k: v.detach().cpu().to(dt) for k, v in G.state_dict().items()}
        nz = noise.detach().cpu().to(dt).requires_grad_(True)
        o = N.generator(sd, styles.detach().cpu().to(dt), hists.detach().cpu().to(dt), nz, L)
        return torch.autograd.grad(o, nz, go.cpu().to(dt))[0]

    ref32 = None
    for fused in (True, False):
        nz = noise.clone().requires_grad_(True)
        rgb, masks = _run_recorded(G, styles, hists, nz, fused)
        g_st, g_hi, g_nz = torch.autograd.grad(rgb, [styles, hists, nz], go)
        assert g_nz is not None and g_nz.shape == noise.shape
        # the same call with a constant noise image: the other gradients are the same bits
        rgb0, _ = _run_recorded(G, styles, hists, noise, fused)
        g_st0, g_hi0 = torch.autograd.grad(rgb0, [styles, hists], go)
        assert torch.equal(rgb, rgb0) and torch.equal(g_st, g_st0) and torch.equal(g_hi, g_hi0)
        with LreluMasks(masks) as lm:
            truth = oracle(torch.float64)
        assert lm.k == len(masks) and lm.flips <= 1e-5 * lm.total and lm.flip_margin <= 2e-6, (lm.flips, lm.total, lm.flip_margin)
        if ref32 is None:
            ref32 = oracle(torch.float32)
        e, rms, rms32 = relmax(_np(g_nz), truth.numpy()), _rms(g_nz.cpu(), truth), _rms(ref32, truth)
        print(f'generator {size, cap, B} fused={fused}: noise gradient relmax {e:.2e} rms {rms:.2e} (fp32 oracle rms {rms32:.2e}, '
              f'relmax {relmax(ref32.numpy(), truth.numpy()):.2e}); flips {lm.flips} of {lm.total}')
        assert e <= 1e-4
        assert rms <= 2 * rms32 + 1e-7


# ---- 4. chain rule between the two noise modes ---------------------------------------------------------------------
def test_noise_image_gradient_is_the_chain_rule_of_the_explicit_noise_mode(gpu_device, monkeypatch):
    from histogan_amd import ops
    from histogan_amd.nets import GeneratorBlock
    dev, B, C, H = gpu_device, 2, 8, 16
    torch.manual_seed(5)
    blk = GeneratorBlock(64, C, C, upsample=False, upsample_rgb=False).to(dev)
    with torch.no_grad():
        for m in (blk.to_noise1, blk.to_noise2):
            m.weight.normal_(std=0.3)
            m.bias.normal_(std=0.1)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, C, H, H, generator=g).to(dev)
    s1, s2, s3 = [(torch.randn(B, C, generator=g) * 0.5).to(dev) for _ in range(3)]
    inoise = torch.rand(B, H, H, 1, generator=g).to(dev)
    gx, grgb = torch.randn(B, C, H, H, generator=g).to(dev), torch.randn(B, 3, H, H, generator=g).to(dev)
    signs = {'a': [], 'b': []}
    # (a) the noise image as the variable
    orig = ops.conv_dnl

    def rec_a(*a):
        out = orig(*a)
        signs['a'].append(out.detach() > 0)
        return out

    monkeypatch.setattr(ops, 'conv_dnl', rec_a)
    nz = inoise.clone().requires_grad_(True)
    xo, rgb = blk.forward_(x, None, s1, s2, s3, inoise=nz)
    got, = torch.autograd.grad((xo * gx).sum() + (rgb * grgb).sum(), nz)
    monkeypatch.setattr(ops, 'conv_dnl', orig)
    # (b) the per-layer noise maps as the variables
    orig_l = F.leaky_relu

    def rec_b(t, *a, **k):
        out = orig_l(t, *a, **k)
        signs['b'].append(out.detach() > 0)
        return out

    with torch.no_grad():
        n1 = blk.to_noise1(inoise).permute(0, 3, 2, 1).contiguous()
        n2 = blk.to_noise2(inoise).permute(0, 3, 2, 1).contiguous()
    n1.requires_grad_(True), n2.requires_grad_(True)
    monkeypatch.setattr(F, 'leaky_relu', rec_b)
    xo_b, rgb_b = blk.forward_(x, None, s1, s2, s3, noise1=n1, noise2=n2)
    monkeypatch.setattr(F, 'leaky_relu', orig_l)
    gn1, gn2 = torch.autograd.grad((xo_b * gx).sum() + (rgb_b * grgb).sum(), [n1, n2])
    assert len(signs['a']) == 2 and len(signs['b']) == 2
    assert all(torch.equal(a, b) for a, b in zip(signs['a'], signs['b'])), 'the two runs took different LeakyReLU branches'
    wn1, wn2 = blk.to_noise1.weight.detach().double().reshape(-1), blk.to_noise2.weight.detach().double().reshape(-1)
    want = torch.einsum('c,bcji->bij', wn1, gn1.double()) + torch.einsum('c,bcji->bij', wn2, gn2.double())
    e = relmax(_np(got[..., 0]), _np(want))
    print(f'chain rule between the noise modes: relmax {e:.2e}')
    assert got.shape == inoise.shape and e <= TOL


# ---- 5. frozen weights -----------------------------------------------------------------------------------------------
# Weight-gradient calls of one backward of Generator(32, 64, 2) with every parameter trainable: conv1 and conv2 of each of
# the L = 4 blocks go through gfused._wgrad once -> 8 conv._direct_wgrad calls, each ending in one conv.conv_wgrad (into
# the flat slot).  The same on the parent commit 38b575e, whose backward made these calls unconditionally.
WGRAD_CALLS_TRAINABLE = 8


def test_frozen_weights_cost_no_weight_gradient(gpu_device, monkeypatch):
    from histogan_amd import conv as C
    from histogan_amd import gfused
    from histogan_amd.optim import FlatParams
    dev = gpu_device
    G = _generator(32, 2, 3, dev)
    flat = FlatParams(list(G.parameters()))
    styles, hists, noise, go = _inputs(G, 3, 3, dev)
    calls = {'wgrad': 0, 'direct': 0, 'after': 0}
    orig_w, orig_d = C.conv_wgrad, C._direct_wgrad

    def count_w(*a, **k):
        calls['wgrad'] += 1
        return orig_w(*a, **k)

    def count_d(*a, **k):
        calls['direct'] += 1
        return orig_d(*a, **k)

    def after():
        calls['after'] += 1

    monkeypatch.setattr(C, 'conv_wgrad', count_w)
    monkeypatch.setattr(C, '_direct_wgrad', count_d)
    monkeypatch.setattr(gfused, 'AFTER_BLOCKS', after)
    res = {}
    for frozen in (True, False):
        for p in G.parameters():
            p.requires_grad_(not frozen)
        flat.zero_grad()
        flat.grad.zero_()
        for k in calls:
            calls[k] = 0
        st, hi = styles.detach().clone().requires_grad_(True), hists.detach().clone().requires_grad_(True)
        nz = noise.clone().requires_grad_(True)
        rgb = G(st, hi, nz)
        assert type(rgb.grad_fn).__name__.startswith('_GeneratorTrain')
        (rgb * go).sum().backward()
        torch.cuda.synchronize()
        res[frozen] = (st.grad, hi.grad, nz.grad)
        assert nz.grad is not None
        if frozen:
            assert calls == {'wgrad': 0, 'direct': 0, 'after': 0}, calls
            assert all(p.grad is None for p in G.parameters())
            assert flat.written == set() and not bool(flat.grad.any())
        else:
            assert calls == {'wgrad': WGRAD_CALLS_TRAINABLE, 'direct': WGRAD_CALLS_TRAINABLE, 'after': 1}, calls
            assert len(flat.written) >= 2 * len(G.blocks) and bool(flat.grad.any())
    for a, b, n in zip(res[True], res[False], ('styles', 'hists', 'noise')):
        assert relmax(_np(a), _np(b)) <= TOL, n


def test_after_blocks_waits_for_weight_gradients_returned_to_autograd(gpu_device, monkeypatch):
    """Two backward passes between zero_grad() and gather() (gradient accumulation).  (a) AFTER_BLOCKS announces that every
    convolution weight of the generator has its final gradient in its flat slot: true after the first pass, not after the
    second, whose to-RGB weight gradients go back to autograd because their slots are already written -- they reach the flat
    buffer only in gather().  (b) After gather() the flat gradient is the sum of the two passes, against the per-block
    autograd path (HG_GFUSED=0), at 1e-5: the tightest bar test_c3_fused_gpu.py holds a weight gradient to (test_gstage_gpu.py's
    fused-versus-per-block comparison of every gradient allows 2e-5)."""
    from histogan_amd import gfused
    from histogan_amd.optim import FlatParams
    dev = gpu_device
    G = _generator(32, 2, 3, dev)
    params = list(G.parameters())
    passes = [_inputs(G, 3, seed, dev) for seed in (3, 4)]
    want = None
    gfused.GFUSED = False
    try:
        for st, hi, nz, go in passes:
            gr = torch.autograd.grad((G(st, hi, nz) * go).sum(), params)
            want = gr if want is None else [a + b for a, b in zip(want, gr)]
    finally:
        gfused.GFUSED = True
    flat = FlatParams(params)
    fired = []
    monkeypatch.setattr(gfused, 'AFTER_BLOCKS', lambda: fired.append(len(flat.written)))
    flat.zero_grad()
    counts = []
    for st, hi, nz, go in passes:
        rgb = G(st, hi, nz)
        assert type(rgb.grad_fn).__name__.startswith('_GeneratorTrain')
        (rgb * go).sum().backward()
        counts.append(len(fired))
    print(f'AFTER_BLOCKS calls after pass 1, 2: {counts}')
    assert counts == [1, 1], counts
    assert fired[0] == 3 * len(G.blocks)                     # conv1, conv2 and to-RGB of every block, written directly
    rgb_w = [b.to_rgb.conv.weight for b in G.blocks]
    assert all(p.grad is not None for p in rgb_w)              # the second pass' to-RGB parts, held by autograd until gather()
    flat.gather()
    torch.cuda.synchronize()
    errs = {n: relmax(_np(p.grad), _np(w)) for (n, p), w in zip(G.named_parameters(), want)}
    print(f'sum of two passes against the per-block path: worst relmax {max(errs.values()):.2e}')
    assert all(p.grad is s.view for p, s in zip(params, flat.slots))
    assert max(errs.values()) <= 1e-5, max(errs.items(), key=lambda kv: kv[1])


# ---- 6. in-place update of the noise image -------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['constant', 'requires_grad', 'no_grad'])
def test_in_place_update_of_the_noise_reaches_the_next_forward(mode, gpu_device):
    import contextlib
    dev = gpu_device
    G = _generator(32, 2, 3, dev)
    styles, hists, noise, _ = _inputs(G, 2, 9, dev)
    noise = noise.clone()
    if mode == 'requires_grad':
        noise.requires_grad_(True)
    ctx = torch.no_grad() if mode == 'no_grad' else contextlib.nullcontext()
    with ctx:
        first = G(styles, hists, noise).detach()
        with torch.no_grad():
            noise.add_(0.25)
        second = G(styles, hists, noise).detach()
        fresh = noise.detach().clone().requires_grad_(mode == 'requires_grad')
        want = G(styles, hists, fresh).detach()
    assert not torch.equal(first, second)
    assert torch.equal(second, want)


# ---- 7. the driver -----------------------------------------------------------------------------------------------------
class _GAN:
    """The three averaged networks project() reads, at Generator(32, 64, 2) size."""

    def __init__(self, dev):
        from histogan_amd.nets import HistVectorizer, StyleVectorizer
        torch.manual_seed(11)
        self.SE = StyleVectorizer(64, 2).to(dev)
        self.HE = HistVectorizer(16, 64, 2).to(dev)
        self.GE = _generator(32, 2, 11, dev)

    def state_dict(self):
        return {f'{n}.{k}': v for n in ('SE', 'HE', 'GE') for k, v in getattr(self, n).state_dict().items()}


@pytest.fixture(scope='module')
def gan_and_image(gpu_device):
    from histogram_classes.RGBuvHistBlock import RGBuvHistBlock
    gan = _GAN(gpu_device)
    image = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(4)).to(gpu_device)
    blk = RGBuvHistBlock(h=16, insz=32, device='cuda')
    with torch.no_grad():
        hist = blk(image)
    return gan, image, blk, hist


@pytest.mark.parametrize('pixel_loss', ['L1', 'L2'])
def test_project_follows_the_oracle_adam_steps(pixel_loss, gan_and_image):
    from histogan_amd.project import project, recolor
    gan, image, blk, hist = gan_and_image
    kw = dict(steps=5, lr=0.05, noise_reg_weight=0.1, style_reg_weight=10.0)
    data, losses, rgb = project(gan, image, pixel_loss=pixel_loss, pixel_loss_weight=1.0, optimize_noise=True,
                                latent_noise=False, hist_block=blk, seed=17, **kw)
    assert set(data) == {'styles', 'in_noise'} and len(losses) == 5
    assert data['styles'].shape == (1, gan.GE.num_layers - 2, 64) and data['in_noise'].shape == (1, 32, 32, 1)
    assert all(p.grad is None and not p.requires_grad for n in ('SE', 'HE', 'GE') for p in getattr(gan, n).parameters())
    t64 = R.projection_oracle(gan.state_dict(), image, hist, 17, pixel_loss, dtype=torch.float64, **kw)
    t32 = R.projection_oracle(gan.state_dict(), image, hist, 17, pixel_loss, dtype=torch.float32, **kw)
    ours = max(abs(a - t) / abs(t) for a, t in zip(losses, t64))
    ref = max(abs(a - t) / abs(t) for a, t in zip(t32, t64))
    print(f'project {pixel_loss}: fp64 losses {[round(v, 4) for v in t64]}; largest relative deviation ours {ours:.2e}, '
          f'fp32 oracle {ref:.2e}')
    assert all(b < a for a, b in zip(t64, t64[1:])), t64
    assert ours <= 2 * ref + 1e-6
    # the generate half with the image's own histogram is the projected image, bit for bit
    assert torch.equal(recolor(gan, data, hist), rgb)
    other = recolor(gan, data, hist.flip(1))
    assert other.shape == rgb.shape and not torch.equal(other, rgb)


def test_project_latent_noise_mode(gan_and_image):
    from histogan_amd.project import project, recolor
    gan, image, blk, hist = gan_and_image
    data, losses, rgb = project(gan, image, steps=1, lr=0.05, optimize_noise=True, latent_noise=True, noise_reg_weight=0.1,
                                style_reg_weight=10.0, hist_block=blk, seed=17)
    L = gan.GE.num_layers
    assert set(data) == {'styles', 'noise1_list', 'noise2_list'} and len(losses) == 1 and np.isfinite(losses[0])
    assert len(data['noise1_list']) == L and len(data['noise2_list']) == L
    for i, (n1, n2) in enumerate(zip(data['noise1_list'], data['noise2_list'])):
        C = gan.GE.blocks[i].to_noise1.out_features
        assert n1.shape == n2.shape == (1, C, 4 << i, 4 << i)
        assert n1.grad is not None and n2.grad is not None and bool(n1.grad.any()) and bool(n2.grad.any())
    assert data['styles'].grad is not None
    assert torch.equal(recolor(gan, data, hist), rgb)
