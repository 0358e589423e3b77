"""The CIE colour difference on the MI355X (hg_delta_e, include/hg_post.h; post.delta_e, post.delta_e_map, project's
delta_e_weight) against the fp64 definition of tests/delta_e_ref.py.

Inputs (delta_e_ref.seeded_pair): t, u = 0.05 + 0.9 rand from one CPU generator, target = t, pred = 0.85 t + 0.15 u, so both
stay inside (0, 1) and no clamping manufactures grey pixels.  The kernel takes one pixel per thread in blocks of 256 and one
finish block of 256 threads per sample, so 300 x 300 (352 partials per sample) is the first listed size at which a finish
thread sums more than one partial.

Condition, asserted on the reference side before anything is compared: no pixel has dE (of either kind) < 1e-2,
min(C'_1, C'_2) < 1e-2 or | 180 - |h'_2 - h'_1| | < 1e-2 degrees -- there dE is not differentiable or a hue branch is within
rounding distance, and two correct fp64 evaluations may disagree.

Bars: both sides evaluate in fp64 from the same fp32 pixels and the kernel rounds once, so map, mean and grad (upstream 1)
are held to 2^-23 max-norm relative (the bar of tests/test_lab_from_rgb_gpu.py for the stand-alone conversions), and the
gradient through autograd with a non-trivial upstream vector to 2^-22 (the product is rounded a second time)."""
import numpy as np
import pytest
import torch

import delta_e_ref as R
import lab_ref
from conftest import relmax

pytestmark = pytest.mark.gpu

TOL = 2.0 ** -23
TOL_AUTOGRAD = 2.0 ** -22

CASES = [(10, (1, 3, 1, 1)), (11, (2, 3, 7, 5)), (12, (2, 3, 16, 24)), (13, (3, 3, 33, 40)), (14, (2, 3, 64, 64)),
         (15, (1, 3, 300, 300))]
_REF = {}


def _case(seed, shape):
    """The inputs of a case and their fp64 references, computed once: {'pred', 'target', (kind): (map, mean, grad)}."""
    if seed not in _REF:
        pred, target = R.seeded_pair(seed, shape)
        assert R.excluded_share(pred, target) == 0.0, R.condition(pred, target)
        _REF[seed] = {'pred': pred, 'target': target, 'cond': R.condition(pred, target)}
        for kind in R.KINDS:
            _REF[seed][kind] = R.fwd_bwd(pred, target, kind)
    return _REF[seed]


def _launch(pred, target, kind, weight=None, want_map=True, want_grad=True):
    from histogan_amd import post
    mean, dmap, grad = post._delta_e_launch(pred, target, weight, kind, want_map, want_grad, 'test')
    return mean, dmap, grad


def _check(tag, got, ref, tol=TOL):
    for name, g, r in zip(('mean', 'map', 'grad'), got, ref):
        if g is None:
            continue
        g = g.cpu()
        assert g.dtype == torch.float32 and g.shape == r.shape and bool(torch.isfinite(g).all()), (tag, name)
        e = relmax(g.numpy(), r.numpy())
        print(f'{tag}: {name} relmax {e:.2e} (bar {tol:.2e})')
        assert e <= tol, (tag, name, e)


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('seed,shape', CASES, ids=[f'{s[2]}x{s[3]}' for _, s in CASES])
def test_map_mean_and_gradient_match_fp64(seed, shape, kind, gpu_device):
    c = _case(seed, shape)
    print(f'condition {shape}: min dE00 {c["cond"][0]:.3f}, min dE76 {c["cond"][1]:.3f}, min C\' {c["cond"][2]:.3f}, hue margin {c["cond"][3]:.3f} deg')
    dmap, mean, grad = c[kind]
    p, t = c['pred'].to(gpu_device), c['target'].to(gpu_device)
    full = _launch(p, t, kind)
    assert full[0].is_contiguous() and full[1].is_contiguous() and full[2].is_contiguous()
    _check(f'dE{kind} {shape}', full, (mean, dmap, grad))
    # every subset of the optional outputs: the same bits, and the mean never changes; a repeat is bit-identical
    for want_map, want_grad in ((False, False), (True, False), (False, True), (True, True)):
        m, d, g = _launch(p, t, kind, want_map=want_map, want_grad=want_grad)
        assert (d is None) == (not want_map) and (g is None) == (not want_grad)
        assert torch.equal(m, full[0])
        assert d is None or torch.equal(d, full[1])
        assert g is None or torch.equal(g, full[2])


@pytest.mark.parametrize('kind', R.KINDS)
def test_input_layouts(kind, gpu_device):
    dev = gpu_device
    # channels-last storage of both images
    c = _case(12, (2, 3, 16, 24))
    cl = lambda x: x.permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2)      # noqa: E731
    p, t = cl(c['pred']), cl(c['target'])
    assert not p.is_contiguous() and not t.is_contiguous()
    got = _launch(p, t, kind)
    _check(f'dE{kind} channels-last', got, (c[kind][1], c[kind][0], c[kind][2]))
    assert torch.equal(got[0], _launch(c['pred'].to(dev), c['target'].to(dev), kind)[0])
    # both images as slices of larger tensors
    c = _case(13, (3, 3, 33, 40))

    def sliced(x, fill):
        big = torch.full((3, 3, 40, 56), fill, device=dev)
        big[:, :, 3:36, 7:47] = x.to(dev)
        return big[:, :, 3:36, 7:47]

    p, t = sliced(c['pred'], float('nan')), sliced(c['target'], 7.0)
    assert not p.is_contiguous()
    _check(f'dE{kind} slices', _launch(p, t, kind), (c[kind][1], c[kind][0], c[kind][2]))


@pytest.mark.parametrize('kind', ['76', '2000', 2000])
def test_autograd_and_public_functions(kind, gpu_device):
    from histogan_amd import post
    dev = gpu_device
    k = int(kind)
    c = _case(13, (3, 3, 33, 40))
    up = torch.tensor([0.7, -1.3, 2.1])
    ref_map, ref_mean, _ = c[k]
    _, _, ref_grad = R.fwd_bwd(c['pred'], c['target'], k, upstream=up)
    p = c['pred'].to(dev).requires_grad_(True)
    t = c['target'].to(dev).requires_grad_(True)           # the target gets no gradient
    out = post.delta_e(p, t, kind)
    assert out.shape == (3,) and out.dtype == torch.float32 and out.requires_grad
    gp, gt = torch.autograd.grad(out, [p, t], up.to(dev), allow_unused=True)
    assert gt is None
    _check(f'delta_e {kind!r}', (out.detach(), None, None), (ref_mean, None, None))
    _check(f'delta_e {kind!r} autograd', (None, None, gp), (None, None, ref_grad), tol=TOL_AUTOGRAD)
    # no graph, and the same mean, when nothing requires grad
    plain = post.delta_e(p.detach(), t.detach(), kind)
    assert not plain.requires_grad and torch.equal(plain, out.detach())
    # the map: never differentiable; (3, H, W) inputs give (H, W) and a 0-dim mean
    dm = post.delta_e_map(p, t, kind)
    assert dm.shape == (3, 33, 40) and not dm.requires_grad
    _check(f'delta_e_map {kind!r}', (None, dm, None), (None, ref_map, None))
    one = post.delta_e_map(p[1], t[1], kind)
    assert one.shape == (33, 40) and torch.equal(one, dm[1])
    single = post.delta_e(p.detach()[1], t.detach()[1], kind)
    assert single.dim() == 0 and torch.equal(single, out.detach()[1])
    # an fp64 prediction gets an fp64 gradient
    p64 = c['pred'].double().to(dev).requires_grad_(True)
    g64, = torch.autograd.grad(post.delta_e(p64, t.detach(), kind).sum(), p64)
    assert g64.dtype == torch.float64
    # srgb_to_lab stays a data-side tool
    with pytest.raises(ValueError, match='from_rgb=True'):
        post.srgb_to_lab(p)


@pytest.mark.parametrize('kind', R.KINDS)
def test_weight_maps(kind, gpu_device):
    from histogan_amd import post
    dev = gpu_device
    c = _case(13, (3, 3, 33, 40))
    pred, target = c['pred'], c['target']
    p, t = pred.to(dev), target.to(dev)
    g = torch.Generator().manual_seed(113)
    frac = torch.rand(3, 33, 40, generator=g) * 1.4 - 0.2              # values below 0 and above 1: clamped
    mask = (torch.rand(3, 33, 40, generator=g) < 0.5).float()
    assert bool((frac < 0).any()) and bool((frac > 1).any()) and 0 < int(mask.sum()) < mask.numel()
    for name, w in (('fractional', frac), ('mask', mask)):
        ref_map, ref_mean, ref_grad = R.fwd_bwd(pred, target, kind, weight=w)
        got = _launch(p, t, kind, weight=w.to(dev))
        _check(f'dE{kind} {name} map', got, (ref_mean, ref_map, ref_grad))
        assert bool((got[2].cpu().permute(1, 0, 2, 3)[:, w.clamp(0, 1) == 0] == 0).all())
        assert torch.equal(got[0], _launch(p, t, kind, weight=w.to(dev), want_map=False, want_grad=False)[0])
        # (B, 1, H, W) maps and strided maps are the same map
        again = _launch(p, t, kind, weight=w.to(dev).unsqueeze(1))
        wide = torch.zeros(3, 33, 80, device=dev)
        wide[:, :, ::2] = w.to(dev)
        strided = _launch(p, t, kind, weight=wide[:, :, ::2])
        for other in (again, strided):
            assert all(torch.equal(a, b) for a, b in zip(got, other))
    # through the public function
    out = post.delta_e(p, t, kind, weight=frac.to(dev))
    _check(f'delta_e({kind}, weight)', (out, None, None), (R.delta_e_mean(pred, target, kind, frac), None, None))
    # an all-zero map: mean 0, gradient 0; a map of ones: the bits of no map
    zero = _launch(p, t, kind, weight=torch.zeros(3, 33, 40, device=dev))
    assert bool((zero[0] == 0).all()) and bool((zero[2] == 0).all()) and bool(torch.isfinite(zero[1]).all())
    ones, none = _launch(p, t, kind, weight=torch.ones(3, 33, 40, device=dev)), _launch(p, t, kind)
    assert all(torch.equal(a, b) for a, b in zip(ones, none))
    with pytest.raises(ValueError, match='weight'):
        post.delta_e(p, t, kind, weight=torch.ones(3, 33, 41, device=dev))


@pytest.mark.parametrize('kind', R.KINDS)
def test_edge_pixels(kind, gpu_device):
    """Anchors, grey, the knee of the transfer curve and components below 0 and above 1, against themselves (every root at
    0) and against a shifted copy.  Forward values are compared; gradients must be finite and exactly 0 on the clamped
    components (no value comparison at the singular pixels)."""
    dev = gpu_device
    e = lab_ref.edge_image()
    out_of_range = (e < 0) | (e > 1)
    assert int(out_of_range.sum()) == 2
    mean, dmap, grad = _launch(e.to(dev), e.to(dev), kind)
    assert bool((mean == 0).all()) and bool((dmap == 0).all()) and bool((grad == 0).all())
    other = e.roll(1, 3)
    ref_map, ref_mean, _ = R.fwd_bwd(e, other, kind)
    mean, dmap, grad = _launch(e.to(dev), other.to(dev), kind)
    _check(f'dE{kind} edge image', (mean, dmap, None), (ref_mean, ref_map, None))
    assert bool(torch.isfinite(grad).all()) and bool(grad.any())
    assert bool((grad.cpu()[out_of_range] == 0).all())


# ---- project ---------------------------------------------------------------------------------------------------------
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
    """The three averaged networks project() reads, at Generator(32, 64, 2) size (as tests/test_noise_grad_gpu.py builds them)."""

    def __init__(self, dev):
        from histogan_amd.nets import HistVectorizer, StyleVectorizer
        torch.manual_seed(11)
        self.SE = StyleVectorizer(64, 2).to(dev)
        self.HE = HistVectorizer(16, 64, 2).to(dev)
        self.GE = _generator(32, 2, 11, dev)

    def state_dict(self):
        return {f'{n}.{k}': v for n in ('SE', 'HE', 'GE') for k, v in getattr(self, n).state_dict().items()}


PROJECT_SEED = 17          # of project's draws; the condition below is asserted for it on the fp64 oracle's renders
PROJECT_KW = dict(steps=5, lr=0.05, noise_reg_weight=0.1, style_reg_weight=10.0)


@pytest.fixture(scope='module')
def gan_and_image(gpu_device):
    from histogram_classes.RGBuvHistBlock import RGBuvHistBlock
    gan = _GAN(gpu_device)
    image = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(4)).to(gpu_device)
    blk = RGBuvHistBlock(h=16, insz=32, device='cuda')
    with torch.no_grad():
        hist = blk(image)
    return gan, image, blk, hist


@pytest.mark.parametrize('kind', ['76', '2000'])
def test_project_with_the_colour_term_follows_the_oracle(kind, gan_and_image):
    from histogan_amd.project import project
    gan, image, blk, hist = gan_and_image
    args = (gan.state_dict(), image, hist, PROJECT_SEED, 'L1')
    t64, renders = R.projection_oracle(*args, delta_e_weight=0.01, delta_e_kind=int(kind), dtype=torch.float64, **PROJECT_KW)
    t32, _ = R.projection_oracle(*args, delta_e_weight=0.01, delta_e_kind=int(kind), dtype=torch.float32, **PROJECT_KW)
    # the condition, on the pixels of the fp64 oracle's five renders whose components are inside [0, 1]
    for i, rgb in enumerate(renders):
        inside = ((rgb >= 0) & (rgb <= 1)).all(dim=1)
        share = R.excluded_share(rgb, image.cpu().double(), mask=inside)
        print(f'render {i}: {int(inside.sum())} of {inside.numel()} pixels inside [0, 1], excluded share {share}')
        assert int(inside.sum()) > 0 and share == 0.0
    data, losses, rgb = project(gan, image, pixel_loss='L1', pixel_loss_weight=1.0, optimize_noise=True, latent_noise=False,
                                hist_block=blk, seed=PROJECT_SEED, delta_e_weight=0.01, delta_e_kind=kind, **PROJECT_KW)
    assert len(losses) == 5 and all(np.isfinite(losses))
    plain, _ = R.projection_oracle(*args, delta_e_weight=0.0, delta_e_kind=int(kind), dtype=torch.float64, **PROJECT_KW)
    assert t64[0] > plain[0] + 1e-3, 'the colour term does not show in the loss'
    ours = max(abs(a - t) / abs(t) for a, t in zip(losses, t64))
    ref = max(abs(a - t) / abs(t) for a, t in zip(t32, t64))
    print(f'project dE{kind}: fp64 losses {[round(v, 4) for v in t64]} (without the term {[round(v, 4) for v in plain]}); '
          f'largest relative deviation ours {ours:.2e}, fp32 oracle {ref:.2e}')
    assert ours <= 2 * ref + 1e-6


def test_project_without_the_colour_term_is_unchanged(gan_and_image, monkeypatch):
    from histogan_amd import post
    from histogan_amd.project import project
    gan, image, blk, hist = gan_and_image
    kw = dict(pixel_loss='L1', hist_block=blk, seed=PROJECT_SEED, **PROJECT_KW)
    _, base, rgb0 = project(gan, image, **kw)

    def boom(*a, **k):
        raise AssertionError('delta_e_weight=0 reached the colour difference')

    monkeypatch.setattr(post, 'delta_e', boom)
    _, off, rgb1 = project(gan, image, delta_e_weight=0, delta_e_kind='2000', **kw)
    assert off == base and torch.equal(rgb0, rgb1)
