"""Test helper (NOT a test module): networks, seeded inputs and oracle gradients for tests/test_flat_grad_paths_gpu.py -- the
gradients that reach an optim.FlatParams buffer, against oracle.histogan_nets on the CPU.

Everything here runs without a GPU (tools/flat_grad_seed_check.py uses it to check the seeds: with the oracle in fp32 standing in
for the run under test, the fp64 oracle on the fp32 run's LeakyReLU branches must meet the caps the GPU tests assert).

A `pass` is a dict: discriminator {x (B, 3, S, S), gl (B,), penalty: bool}; generator {t: the 3 L projected styles, noise
(B, S, S, 1), gout (B, 3, S, S)}.  Each is driven by a FIXED upstream gradient, (out * g).sum(): no hinge, no extra kink.
"""
import zlib

import torch
import torch.nn.functional as F

from oracle import histogan_nets as N
from oracle_step import LreluMasks

B, SIZE, CAP, LATENT = 3, 32, 2, 512
FLIP_SHARE, FLIP_MARGIN = 1e-5, 2e-6        # the caps of tests/test_operand_layout_gpu.py, tests/test_noise_grad_gpu.py


def cpu_gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def discriminator():
    from histogan_amd.nets import Discriminator
    torch.manual_seed(13)
    return Discriminator(SIZE, CAP)


def generator():
    from histogan_amd.nets import Generator
    torch.manual_seed(11)
    G = Generator(SIZE, LATENT, network_capacity=CAP)
    with torch.no_grad():
        for b in G.blocks:                      # (the reference initialises the noise projections to zero: make them count)
            for m in (b.to_noise1, b.to_noise2):
                m.weight.normal_(std=0.3)
                m.bias.normal_(std=0.1)
    return G


def d_pass(key, kind='fake', penalty=False):
    """A discriminator pass: 'real'-like images in [0, 1], 'fake'-like ones normal around 0.5 (what a young generator emits)."""
    g = cpu_gen('d_pass', key)
    x = torch.rand(B, 3, SIZE, SIZE, generator=g) if kind == 'real' else 0.5 + 0.5 * torch.randn(B, 3, SIZE, SIZE, generator=g)
    return dict(x=x, gl=torch.randn(B, generator=g), penalty=penalty)


def g_pass(key, G):
    """A generator pass; the projected styles come from G's own to_style layers (fp32, on the CPU: the same tensors everywhere)."""
    g = cpu_gen('g_pass', key)
    L = G.num_layers
    sty = torch.randn(L, B, LATENT, generator=g)
    with torch.no_grad():
        t = [F.linear(sty[i], m.weight.detach().cpu(), m.bias.detach().cpu())
             for i, b in enumerate(G.blocks) for m in (b.to_style1, b.to_style2, b.to_rgb.to_style)]
    return dict(t=t, noise=torch.rand(B, SIZE, SIZE, 1, generator=g), gout=torch.randn(B, 3, SIZE, SIZE, generator=g))


class OracleBranches:
    """While active, records the branch (pre-activation > 0) of every feature-map LeakyReLU of the oracle networks, in call order:
    an oracle run in fp32 then yields the `masks` a run under test would."""

    def __enter__(self):
        self.masks, self._orig = [], N.lrelu

        def hooked(x):
            if x.dim() == 4:
                self.masks.append(x.detach() > 0)
            return self._orig(x)

        N.lrelu = hooked
        return self.masks

    def __exit__(self, *exc):
        N.lrelu = self._orig
        return False


def _caps(lm, masks, what):
    assert lm.k == len(masks), (what, lm.k, len(masks))
    assert lm.flips <= FLIP_SHARE * lm.total and lm.flip_margin <= FLIP_MARGIN, (what, lm.flips, lm.total, lm.flip_margin)


def _state(module, dtype):
    return {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in module.state_dict().items()}


def d_loss(sd, p, masks, dtype=torch.float64, scale=1.0):
    """scale * ((D(x) * gl).sum() [+ gradient penalty on x]) with the oracle, on the branches `masks` (None: its own)."""
    x = p['x'].to(dtype).requires_grad_(p['penalty'])
    nblk = sum(1 for k in sd if k.endswith('conv_res.weight'))
    if masks is None:
        out = N.discriminator(sd, x, nblk)
    else:
        with LreluMasks(masks) as lm:
            out = N.discriminator(sd, x, nblk)
        _caps(lm, masks, 'discriminator')
    loss = (out * p['gl'].to(dtype)).sum()
    if p['penalty']:
        loss = loss + N.gradient_penalty(x, out)
    return loss * scale


def d_truth(D, passes, masks, scales=None, dtype=torch.float64, frozen=()):
    """{parameter name: d / d parameter of sum_i scales[i] * d_loss(pass i)} with the oracle in `dtype`; names starting with
    one of `frozen` get zeros (no loss reaches them in the run under test)."""
    sd = _state(D, dtype)
    scales = scales or [1.0] * len(passes)
    total = sum(d_loss(sd, p, m, dtype, s) for p, m, s in zip(passes, masks, scales))
    names = [n for n, _ in D.named_parameters()]
    live = [n for n in names if not n.startswith(tuple(frozen))] if frozen else names
    gr = dict(zip(live, torch.autograd.grad(total, [sd[n] for n in live])))
    return {n: gr[n].detach() if n in gr else torch.zeros_like(sd[n]).detach() for n in names}


def d_branches(D, p):
    """The branches the oracle itself takes in fp32 on pass p (stand-in for a run under test)."""
    sd = _state(D, torch.float32)
    with OracleBranches() as masks, torch.no_grad():
        N.discriminator(sd, p['x'], sum(1 for k in sd if k.endswith('conv_res.weight')))
    return [m.clone() for m in masks]


STYLE_LAYERS = ('to_style1', 'to_style2', 'to_rgb.to_style')


def _g_state(G, p, dtype):
    """G's state for the oracle with the projected styles of pass p as INPUTS: the oracle projects its style vectors itself,
    so sample b gets the unit vector e_b as its style and every to_style layer the weight [t^T, 0] and bias 0 -- the projection
    is then t[b], exactly, and its gradient the first B columns of the weight's."""
    sd = _state(G, dtype)
    nb = p['t'][0].shape[0]
    for i in range(len(G.blocks)):
        for j, lay in enumerate(STYLE_LAYERS):
            t = p['t'][3 * i + j].to(dtype)
            w = torch.zeros(t.shape[1], LATENT, dtype=dtype)
            w[:, :nb] = t.t()
            sd[f'blocks.{i}.{lay}.weight'] = w.requires_grad_(True)
            sd[f'blocks.{i}.{lay}.bias'] = torch.zeros(t.shape[1], dtype=dtype)
    return sd


def g_out(G, sd, p, masks, dtype):
    nb, L = p['t'][0].shape[0], G.num_layers
    eye = torch.eye(nb, LATENT, dtype=dtype)
    styles, hists = eye[:, None, :].expand(nb, L - 2, LATENT), eye[:, None, :].expand(nb, 2, LATENT)
    if masks is None:
        return N.generator(sd, styles, hists, p['noise'].to(dtype), L)
    with LreluMasks(masks) as lm:
        out = N.generator(sd, styles, hists, p['noise'].to(dtype), L)
    _caps(lm, masks, 'generator')
    return out


def g_truth(G, passes, masks, dtype=torch.float64):
    """-> ({parameter name: gradient of sum_i (G(pass i) * gout_i).sum()}, [per pass: the gradients of its projected styles],
    [per pass: the image]).  The to_style layers get zeros: with the projected styles as inputs no loss reaches them."""
    names = [n for n, _ in G.named_parameters()]
    live = [n for n in names if not any(('.' + lay + '.') in n for lay in STYLE_LAYERS)]
    grads = {n: 0.0 for n in live}
    gts, imgs = [], []
    for p, m in zip(passes, masks):
        sd = _g_state(G, p, dtype)
        out = g_out(G, sd, p, m, dtype)
        sty = [f'blocks.{i}.{lay}.weight' for i in range(len(G.blocks)) for lay in STYLE_LAYERS]
        gr = torch.autograd.grad(out, [sd[n] for n in live + sty], p['gout'].to(dtype))
        for n, g in zip(live, gr):
            grads[n] = grads[n] + g.detach()
        nb = p['t'][0].shape[0]
        gts.append([g.detach()[:, :nb].t().contiguous() for g in gr[len(live):]])
        imgs.append(out.detach())
    sd0 = G.state_dict()
    return {n: grads[n] if n in grads else torch.zeros_like(sd0[n], dtype=dtype, device='cpu') for n in names}, gts, imgs


def g_branches(G, p):
    with OracleBranches() as masks, torch.no_grad():
        g_out(G, _g_state(G, p, torch.float32), p, None, torch.float32)
    return [m.clone() for m in masks]


def relmax_t(a, b):
    """max |a - b| / max |b| (conftest.relmax) on tensors."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    den = float(b.abs().max()) if b.numel() else 0.0
    return float((a - b).abs().max()) / (den if den > 0 else 1.0) if b.numel() else 0.0


def worst(got, want):
    """(name, relmax) of the parameter furthest from `want`, over the names of `want`."""
    errs = {n: relmax_t(got[n], want[n]) for n in want}
    n = max(errs, key=errs.get)
    return n, errs[n], errs


# Input draws per scenario, picked on the CPU with the fp64 oracle alone (tools/flat_grad_seed_check.py) for the distance of the
# closest LeakyReLU pre-activation from zero: >= 8e-6 of its layer's maximum everywhere, where fp32 evaluations differ by ~1e-7.
DRAW = {'both_routes': 1, 'penalty': 1}
G_DRAWS = ('g', 'h')


def d_scenario(name):
    """(passes, scales) of a discriminator scenario of tests/test_flat_grad_paths_gpu.py."""
    key = lambda i: (name, i, DRAW[name]) if name in DRAW else (name, i)
    if name == 'plain':
        return [d_pass('plain')], [1.0]
    if name in ('two_passes', 'both_routes', 'unreached'):
        return [d_pass(key(0), 'fake'), d_pass(key(1), 'real')], [1.0, 1.0]
    if name == 'penalty':
        return [d_pass(key(0), 'fake'), d_pass(key(1), 'real', penalty=True)], [1.0, 1.0]
    if name == 'accumulation':
        return [d_pass(key(i), 'real' if i % 2 else 'fake') for i in range(3)], [1.0 / 3] * 3
    raise KeyError(name)


def g_scenario(G):
    return [g_pass(k, G) for k in G_DRAWS]


D_SCENARIOS = ('plain', 'two_passes', 'penalty', 'accumulation', 'both_routes', 'unreached')
