"""SSIM / MS-SSIM on the MI355X (hg_ssim_fwd, hg_ssim_bwd, include/hg_post.h; post.ssim, post.ssim_map, post.ms_ssim, project's
ssim_weight, reconstruction_loss('SSIM')) against the fp64 definition of tests/ssim_ref.py.

Inputs (ssim_ref.seeded_pair): t, u = 0.05 + 0.9 rand from one CPU generator, target = t, pred = 0.85 t + 0.15 u, so nothing is
clamped and the sRGB knee is never met; nothing is excluded.  The shapes follow from the kernel's structure, with T =
post.SSIM_TILE the edge of a workgroup's tile (of the map in the forward, of the input in the backward) and
post.SSIM_FINISH_THREADS the threads that sum a sample's tile partials; every case asserts that it reaches what it is there for.

Bars: both sides evaluate in fp64 from the same fp32 pixels and the kernel rounds once, so map, means, MS-SSIM and the
gradients with upstream ones are held to 2^-23 max-norm relative (conftest.relmax), and to 2^-22 where autograd multiplies by
an fp32 upstream afterwards -- the bars of tests/test_delta_e_gpu.py, for the same reason."""
import numpy as np
import pytest
import torch

import ssim_ref as R
from conftest import relmax

pytestmark = pytest.mark.gpu

TOL = 2.0 ** -23
TOL_AUTOGRAD = 2.0 ** -22


def _consts():
    from histogan_amd import post
    return post.SSIM_TILE, post.SSIM_FINISH_THREADS


def _tiles(n, T):
    return -(-n // T)


def _first_finish_size(T, F):
    """The first square size whose map has more tiles than the finish block has threads."""
    n = 11
    while _tiles(n - 10, T) ** 2 <= F:
        n += 1
    return n


# name -> (seed, shape as a function of (T, F)); the assertions on what a shape reaches are in test_shapes_reach_their_structure
CASES = {
    'one-position': (20, lambda T, F: (1, 3, 11, 11)),
    'small': (21, lambda T, F: (2, 3, 12, 17)),
    'one-tile': (22, lambda T, F: (1, 3, T + 10, T + 10)),
    'ragged': (23, lambda T, F: (2, 3, T + 11, 2 * T + 13)),
    'batch3': (24, lambda T, F: (3, 3, 20, 23)),
    'finish': (25, lambda T, F: (1, 3, _first_finish_size(T, F), _first_finish_size(T, F))),
}
_REF = {}


def _case(name):
    """The inputs of a case and their fp64 references, computed once and left unchanged."""
    if name not in _REF:
        seed, shape = CASES[name]
        shape = shape(*_consts())
        pred, target = R.seeded_pair(seed, shape)
        c = {'pred': pred, 'target': target, 'shape': shape}
        for ch in R.CHANNELS:
            s, cs = R.ssim_means(pred, target, ch)
            _, g_s = R.fwd_bwd(pred, target, ch, kind='ssim')
            _, g_c = R.fwd_bwd(pred, target, ch, kind='cs')
            c[ch] = {'map': R.ssim_map(pred, target, ch), 'means': torch.stack((s, cs), dim=1), 'grad_ssim': g_s, 'grad_cs': g_c}
        _REF[name] = c
    return _REF[name]


def _mode(ch):
    from histogan_amd import post
    return post.ssim_channels(ch)


def _fwd(p, t, ch, **kw):
    from histogan_amd import post
    return post._ssim_fwd(p, t, _mode(ch), **kw)


def _bwd(p, t, ch, a, c):
    from histogan_amd import post
    coef = torch.tensor([[a, c]] * p.shape[0], dtype=torch.float64, device=p.device)
    return post._ssim_bwd(p, t, _mode(ch), coef)


def _check(tag, got, ref, tol=TOL, dtype=torch.float32):
    g = got.detach().cpu()
    assert g.dtype == dtype and g.shape == ref.shape and bool(torch.isfinite(g).all()), (tag, g.dtype, g.shape, ref.shape)
    e = relmax(g.numpy(), ref.numpy())
    print(f'{tag}: relmax {e:.2e} (bar {tol:.2e})')
    assert e <= tol, (tag, e)
    return e


def test_shapes_reach_their_structure():
    T, F = _consts()
    sh = {k: v[1](T, F) for k, v in CASES.items()}
    assert sh['one-position'][2:] == (11, 11)                                                  # a 1 x 1 map
    H, W = sh['one-tile'][2:]
    assert _tiles(H - 10, T) == _tiles(W - 10, T) == 1 and (H - 10) % T == 0 and _tiles(H, T) == 2   # a full map tile; input tiles with halo
    H, W = sh['ragged'][2:]
    assert (_tiles(H - 10, T), _tiles(W - 10, T)) == (2, 3) and (H - 10) % T == 1 and (W - 10) % T == 3   # ragged last map tiles
    assert (_tiles(H, T), _tiles(W, T)) == (2, 3) and H % T and W % T and W > 2 * T + 10          # an input tile with halo inside on both sides
    assert sh['batch3'][0] == 3
    n = sh['finish'][2]
    assert _tiles(n - 10, T) ** 2 > F >= _tiles(n - 11, T) ** 2                                  # a finish thread sums two partials: first size


@pytest.mark.parametrize('ch', R.CHANNELS)
@pytest.mark.parametrize('name', list(CASES))
def test_map_means_and_gradient_match_fp64(name, ch, gpu_device):
    c = _case(name)
    ref = c[ch]
    p, t = c['pred'].to(gpu_device), c['target'].to(gpu_device)
    means, smap, pools = _fwd(p, t, ch, want_map=True, want_pool=True)
    assert means.is_contiguous() and smap.is_contiguous()
    tag = f'ssim {ch} {c["shape"]}'
    _check(f'{tag} means', means, ref['means'], dtype=torch.float64)
    _check(f'{tag} map', smap, ref['map'])
    # the pooled planes are F.avg_pool2d of the reference's planes (fp64, nothing rounded)
    for got, img in zip(pools, (c['pred'], c['target'])):
        want = torch.nn.functional.avg_pool2d(R.planes(img, ch), 2)
        assert got.shape == want.shape and got.dtype == torch.float64
        if want.numel():
            assert relmax(got.cpu().numpy(), want.numpy()) <= 1e-14
    g_s, g_c = _bwd(p, t, ch, 1.0, 0.0), _bwd(p, t, ch, 0.0, 1.0)
    _check(f'{tag} grad of mean ssim', g_s, ref['grad_ssim'])
    _check(f'{tag} grad of mean cs', g_c, ref['grad_cs'])
    # every subset of the optional outputs: the same bits, and the means never change; a repeat is bit-identical
    for want_map, want_pool in ((False, False), (True, False), (False, True), (True, True)):
        m, s, q = _fwd(p, t, ch, want_map=want_map, want_pool=want_pool)
        assert (s is None) == (not want_map) and (q is None) == (not want_pool)
        assert torch.equal(m, means)
        assert s is None or torch.equal(s, smap)
        assert q is None or (torch.equal(q[0], pools[0]) and torch.equal(q[1], pools[1]))
    assert torch.equal(_bwd(p, t, ch, 1.0, 0.0), g_s)


@pytest.mark.parametrize('ch', R.CHANNELS)
def test_input_layouts(ch, gpu_device):
    dev = gpu_device
    c = _case('ragged')
    ref = c[ch]
    plain = _fwd(c['pred'].to(dev), c['target'].to(dev), ch, want_map=True)
    # channels-last storage of both images
    cl = lambda x: x.permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2)      # noqa: E731
    p, t = cl(c['pred']), cl(c['target'])
    assert not p.is_contiguous() and not t.is_contiguous()
    means, smap, _ = _fwd(p, t, ch, want_map=True)
    assert torch.equal(means, plain[0]) and torch.equal(smap, plain[1])
    _check(f'ssim {ch} channels-last grad', _bwd(p, t, ch, 1.0, 0.0), ref['grad_ssim'])
    # both images as slices of larger tensors
    B, _, H, W = c['shape']

    def sliced(x, fill):
        big = torch.full((B, 3, H + 9, W + 16), fill, device=dev)
        big[:, :, 3:3 + H, 7:7 + W] = x.to(dev)
        return big[:, :, 3:3 + H, 7:7 + W]

    p, t = sliced(c['pred'], float('nan')), sliced(c['target'], 7.0)
    assert not p.is_contiguous()
    means, smap, _ = _fwd(p, t, ch, want_map=True)
    assert torch.equal(means, plain[0]) and torch.equal(smap, plain[1])
    _check(f'ssim {ch} slices grad', _bwd(p, t, ch, 1.0, 0.0), ref['grad_ssim'])


@pytest.mark.parametrize('ch', R.CHANNELS)
def test_out_of_range_equal_and_near_flat_images(ch, gpu_device):
    from histogan_amd import post
    dev = gpu_device
    T, _ = _consts()
    shape = (2, 3, T + 11, T + 15)
    # out-of-range pixels: the clamp's mask on the gradient, finite everywhere
    pred, target = R.seeded_pair(30, shape)
    pred, target = pred * 1.3 - 0.15, target * 1.3 - 0.15
    outside = (pred < 0) | (pred > 1)
    assert 0 < int(outside.sum()) < outside.numel() // 2
    ref, ref_g = R.fwd_bwd(pred, target, ch)
    p, t = pred.to(dev), target.to(dev)
    means, smap, _ = _fwd(p, t, ch, want_map=True)
    _check(f'ssim {ch} out of range: mean', means[:, 0], ref, dtype=torch.float64)
    _check(f'ssim {ch} out of range: map', smap, R.ssim_map(pred, target, ch))
    g = _bwd(p, t, ch, 1.0, 0.0)
    _check(f'ssim {ch} out of range: grad', g, ref_g)
    assert bool((g.cpu()[outside] == 0).all()) and bool(g.cpu()[~outside].any())
    # equal images: exactly 1, gradient exactly 0 (also through MS-SSIM's five levels)
    means, smap, _ = _fwd(t, t.clone(), ch, want_map=True)
    assert bool((means == 1).all()) and bool((smap == 1).all())
    assert bool((_bwd(t, t.clone(), ch, 1.0, 0.0) == 0).all()) and bool((_bwd(t, t.clone(), ch, 0.3, -0.7) == 0).all())
    big = R.seeded_pair(31, (1, 3, 177, 176))[1].to(dev).requires_grad_(True)
    ms = post.ms_ssim(big, big.detach().clone(), ch)
    g, = torch.autograd.grad(ms.sum(), big)
    assert bool((ms == 1).all()) and bool((g == 0).all())
    # the near-flat bright pair: sigma^2 = E[x^2] - mu^2 cancels seven digits, and C2 = 9e-4 does not hide an fp32 rounding
    pred, target = R.near_flat_pair(32, (1, 3, 37, 45))
    ref, ref_g = R.fwd_bwd(pred, target, ch)
    p, t = pred.to(dev), target.to(dev)
    means, smap, _ = _fwd(p, t, ch, want_map=True)
    _check(f'ssim {ch} near-flat: mean', means[:, 0], ref, dtype=torch.float64)
    _check(f'ssim {ch} near-flat: map', smap, R.ssim_map(pred, target, ch))
    _check(f'ssim {ch} near-flat: grad', _bwd(p, t, ch, 1.0, 0.0), ref_g)


MS_SHAPES = [(40, (1, 3, 176, 176)), (41, (1, 3, 183, 201)), (42, (2, 3, 191, 176))]


@pytest.mark.parametrize('ch', R.CHANNELS)
@pytest.mark.parametrize('seed,shape', MS_SHAPES, ids=[f'{s[2]}x{s[3]}' for _, s in MS_SHAPES])
def test_ms_ssim(seed, shape, ch, gpu_device):
    from histogan_amd import post
    pred, target = R.seeded_pair(seed, shape)
    lv = R.ms_ssim_levels(pred, target, ch)
    odd = sum(1 for _, _, (h, w) in lv[:-1] if h % 2 or w % 2)
    print(f'ms-ssim {ch} {shape}: level sizes {[s for _, _, s in lv]} ({odd} levels drop a row or column), reference cs means '
          f'{[round(float(cs.min()), 4) for _, cs, _ in lv]}')
    assert min(lv[-1][2]) == 11 and (odd >= 2 or shape[2:] == (176, 176))
    assert all(float(cs.min()) > 0.9 for _, cs, _ in lv) and float(lv[-1][0].min()) > 0.9      # far from the clamp
    ref, ref_g = R.fwd_bwd(pred, target, ch, kind='ms-ssim')
    p = pred.to(gpu_device).requires_grad_(True)
    t = target.to(gpu_device)
    ms = post.ms_ssim(p, t, ch)
    assert ms.shape == (shape[0],) and ms.requires_grad
    g, = torch.autograd.grad(ms.sum(), p)
    _check(f'ms-ssim {ch} {shape}', ms, ref)
    _check(f'ms-ssim {ch} {shape} grad', g, ref_g)
    again = post.ms_ssim(p, t, ch)
    g2, = torch.autograd.grad(again.sum(), p)
    assert torch.equal(again, ms) and torch.equal(g2, g)
    if shape[0] > 1:                                   # a non-trivial upstream vector
        up = torch.tensor([0.7, -1.3])
        _, ref_u = R.fwd_bwd(pred, target, ch, upstream=up, kind='ms-ssim')
        gu, = torch.autograd.grad(post.ms_ssim(p, t, ch), p, up.to(gpu_device))
        _check(f'ms-ssim {ch} {shape} grad, upstream {up.tolist()}', gu, ref_u, tol=TOL_AUTOGRAD)


@pytest.mark.parametrize('ch', R.CHANNELS)
def test_autograd_and_public_functions(ch, gpu_device):
    from histogan_amd import post
    dev = gpu_device
    c = _case('batch3')
    up = torch.tensor([0.7, -1.3, 2.1])
    _, ref_grad = R.fwd_bwd(c['pred'], c['target'], ch, upstream=up)
    p = c['pred'].to(dev).requires_grad_(True)
    t = c['target'].to(dev).requires_grad_(True)           # the target gets no gradient
    out = post.ssim(p, t, ch)
    assert out.shape == (3,) and out.dtype == torch.float32 and out.requires_grad
    gp, gt = torch.autograd.grad(out, [p, t], up.to(dev), allow_unused=True)
    assert gt is None
    _check(f'ssim {ch!r}', out, c[ch]['means'][:, 0])
    _check(f'ssim {ch!r} autograd', gp, ref_grad, tol=TOL_AUTOGRAD)
    # no graph, and the same mean, when nothing requires grad; the default is 'L'
    plain = post.ssim(p.detach(), t.detach(), ch)
    assert not plain.requires_grad and torch.equal(plain, out.detach())
    assert torch.equal(post.ssim(p.detach(), t.detach()), post.ssim(p.detach(), t.detach(), 'L'))
    # the map: never differentiable; (3, H, W) inputs give (H - 10, W - 10) and a 0-dim mean
    B, _, H, W = c['shape']
    sm = post.ssim_map(p, t, ch)
    assert sm.shape == (B, H - 10, W - 10) and not sm.requires_grad
    _check(f'ssim_map {ch!r}', sm, c[ch]['map'])
    one = post.ssim_map(p[1], t[1], ch)
    assert one.shape == (H - 10, W - 10) and torch.equal(one, sm[1])
    single = post.ssim(p.detach()[1], t.detach()[1], ch)
    assert single.dim() == 0 and torch.equal(single, out.detach()[1])
    # an fp64 prediction gets an fp64 gradient
    p64 = c['pred'].double().to(dev).requires_grad_(True)
    g64, = torch.autograd.grad(post.ssim(p64, t.detach(), ch).sum(), p64)
    assert g64.dtype == torch.float64


# ---- users -----------------------------------------------------------------------------------------------------------
def test_reconstruction_loss_ssim(gpu_device):
    from histogan_amd.retrainer import reconstruction_loss
    dev = gpu_device
    pred, target = R.seeded_pair(50, (2, 3, 40, 52))
    v, g = R.fwd_bwd(pred, target, 'L')
    want, want_g = (1 - v).mean(), -g / 2
    # the trainer's order: compute_loss(input image, generated image); the gradient reaches the second argument
    gen = pred.to(dev).requires_grad_(True)
    loss = reconstruction_loss('SSIM').compute_loss(target.to(dev), gen)
    grad, = torch.autograd.grad(loss, gen)
    # the loss is 1 - (an fp32 number near 1): post.ssim's rounding, 2^-24 absolute, is 2^-24 / loss relative to the loss; the
    # fp32 subtraction is exact there (Sterbenz) and the mean of two rounds once more
    _check('reconstruction_loss(SSIM)', loss, want.reshape(()), tol=2.0 ** -24 / float(want) + 2.0 ** -24)
    _check('reconstruction_loss(SSIM) grad', grad, want_g, tol=TOL_AUTOGRAD)
    # a fourth channel is ignored
    four = torch.cat((pred, torch.zeros(2, 1, 40, 52)), dim=1).to(dev)
    assert torch.equal(reconstruction_loss('SSIM').compute_loss(torch.cat((target, torch.ones(2, 1, 40, 52)), dim=1).to(dev), four), loss.detach())


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


class _GAN:
    """The three averaged networks project() reads, at Generator(32, 64, 2) size (as tests/test_delta_e_gpu.py builds them)."""

    def __init__(self, dev):
        from histogan_amd.nets import HistVectorizer, StyleVectorizer
        torch.manual_seed(11)
        self.SE = StyleVectorizer(64, 2).to(dev)
        self.HE = HistVectorizer(16, 64, 2).to(dev)
        self.GE = _generator(32, 2, 11, dev)

    def state_dict(self):
        return {f'{n}.{k}': v for n in ('SE', 'HE', 'GE') for k, v in getattr(self, n).state_dict().items()}


PROJECT_KW = dict(steps=2, lr=0.05, noise_reg_weight=0.1, style_reg_weight=10.0)


def test_project_with_the_structure_term(gpu_device, monkeypatch):
    """project(steps=2, ssim_weight=0.5) against the same Adam loop on the fp64 oracle networks with the loss composed from
    tests/ssim_ref.py.  The bar is the reference's own error, as for the colour term: twice what the same oracle in fp32
    deviates from it.  With ssim_weight=0 nothing of SSIM is reached and the result is that of a call without the argument."""
    from histogan_amd import post
    from histogan_amd.project import project
    from histogram_classes.RGBuvHistBlock import RGBuvHistBlock
    gan = _GAN(gpu_device)
    image = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(4)).to(gpu_device)
    blk = RGBuvHistBlock(h=16, insz=32, device='cuda')
    with torch.no_grad():
        hist = blk(image)
    args = (gan.state_dict(), image, hist, 17, 'L1')
    t64 = R.projection_oracle(*args, ssim_weight=0.5, dtype=torch.float64, **PROJECT_KW)
    t32 = R.projection_oracle(*args, ssim_weight=0.5, dtype=torch.float32, **PROJECT_KW)
    plain = R.projection_oracle(*args, ssim_weight=0.0, dtype=torch.float64, **PROJECT_KW)
    kw = dict(pixel_loss='L1', hist_block=blk, seed=17, **PROJECT_KW)
    _, losses, _ = project(gan, image, ssim_weight=0.5, **kw)
    assert len(losses) == 2 and all(np.isfinite(losses))
    assert t64[0] > plain[0] + 1e-2, 'the structure term does not show in the loss'
    ours = max(abs(a - t) / abs(t) for a, t in zip(losses, t64))
    ref = max(abs(a - t) / abs(t) for a, t in zip(t32, t64))
    print(f'project ssim: fp64 losses {[round(v, 5) for v in t64]} (without the term {[round(v, 5) for v in plain]}); '
          f'largest relative deviation ours {ours:.2e}, fp32 oracle {ref:.2e}')
    assert ours <= 2 * ref + 1e-6
    _, base, rgb0 = project(gan, image, **kw)

    def boom(*a, **k):
        raise AssertionError('ssim_weight=0 reached SSIM')

    monkeypatch.setattr(post, 'ssim', boom)
    monkeypatch.setattr(post, 'ms_ssim', boom)
    _, off, rgb1 = project(gan, image, ssim_weight=0, ssim_kind='ms-ssim', **kw)
    assert off == base and torch.equal(rgb0, rgb1)
