"""hellinger_loss (histogan_amd/csrc/hg_hellinger.hip) beyond its block cap, against the reference's inline formula
(histoGAN/histoGAN.py:957-960) evaluated in fp64 from the same fp32 inputs, and that formula's fp64 autograd gradient.

The launcher runs min(ceil(n / 1024), 1024) blocks of 256 threads: every thread of k_hell_partial and of k_hell_final's
gradient loop walks a grid-stride loop, and above n = 1024 * 1024 the grid no longer grows with n, so the loops make
more than four trips, the last one ragged when n is odd; k_hell_final then sums 1024 partials, four per thread.  The other
tests of the loss stop at n = 49 152 (48 blocks).  Every case asserts, from its shape alone, what it reaches.
"""
import json
import math

import pytest
import torch

from conftest import relmax

pytestmark = pytest.mark.gpu

E_LOSS, E_GRAD = 1e-6, 1e-5      # the bars of test_hist_gpu.py::test_hellinger_inline_formula_matches_kernel
CAP = 1024                       # kMaxBlocks, and the elements one block covers without another trip


def _blocks(n):
    return min(max((n + 1023) // 1024, 1), CAP)


CASES = [
    # (B, P, h), what the shape must reach
    ((5, 3, 271), lambda n: n > CAP * 1024 and n % 2 == 1 and n % 256 != 0 and _blocks(n) == CAP),
    ((6, 3, 256), lambda n: n > CAP * 1024 and n % 1024 == 0 and _blocks(n) == CAP and n < 5 * CAP * 256),
    ((4, 3, 256), lambda n: n < CAP * 1024 and _blocks(n) == 768),
    ((1, 1, 1), lambda n: n == 1 and _blocks(n) == 1),
    ((3, 1, 19), lambda n: _blocks(n) == 2 and n % 256 != 0),
    ((32, 3, 64), lambda n: n == 393216 and _blocks(n) == 384),        # the call bench.py makes
]


def _record(record_testsuite_property, key, val):
    """A case's measured errors as a test-suite property (kept by pytest --junitxml), and on stdout."""
    print(f'{key}: {json.dumps(val, sort_keys=True)}')
    record_testsuite_property(key, json.dumps(val, sort_keys=True))


@pytest.fixture(scope='module')
def hists():
    """Per shape: L1-normalised random positive target and generated histograms (fp32, CPU), shared by both alphas.
    Bins in [0.05, 1.05) before the normalisation: sqrt(t / g) <= 4.6, so the gradient's largest element, which relmax
    divides by, is within an order of magnitude of the typical one.  The single bin of (1, 1, 1) is left as drawn: normalised
    it is exactly 1 in both histograms, where the loss is 0 and its gradient 0/0 as in the reference."""
    out = {}
    for (B, P, h), _ in CASES:
        g = torch.Generator().manual_seed(B * 1000003 + P * 1009 + h)
        t, gen = (torch.rand(B, P, h, h, generator=g) + 0.05 for _ in range(2))
        if t.numel() > 1:
            t, gen = t / t.sum(dim=(1, 2, 3), keepdim=True), gen / gen.sum(dim=(1, 2, 3), keepdim=True)
        out[B, P, h] = t, gen
    return out


@pytest.mark.parametrize('alpha', [2.0, 1 / 32], ids=['alpha2', 'alpha1_32'])
@pytest.mark.parametrize('shape,reach', CASES, ids=['x'.join(map(str, s)) for s, _ in CASES])
def test_hellinger_matches_fp64(shape, reach, alpha, hists, gpu_device, record_testsuite_property):
    """Loss within 1e-6 absolute, gradient within 1e-5 relmax; no gradient for the target; a repeat call is bit-equal; an
    upstream gradient scales the result exactly (`grad * gl` of HellingerFunction.backward)."""
    from histogan_amd.hist import hellinger_loss
    B, P, h = shape
    n = B * P * h * h
    assert reach(n), (shape, n)
    t, gen = hists[shape]

    td, gd = t.double(), gen.double().requires_grad_(True)
    ref = alpha * (1 / math.sqrt(2.0)) * torch.sqrt(torch.sum(torch.pow(torch.sqrt(td) - torch.sqrt(gd), 2))) / B
    gref, = torch.autograd.grad(ref, gd)
    ref = float(ref.detach())

    tg = t.to(gpu_device).requires_grad_(True)
    gg = gen.to(gpu_device).requires_grad_(True)
    loss = hellinger_loss(tg, gg, alpha)
    (loss * 0.37).backward()
    grad_scaled, grad_target = gg.grad, tg.grad
    grad, = torch.autograd.grad(hellinger_loss(tg, gg, alpha), gg)
    loss2 = hellinger_loss(tg, gg, alpha)
    grad2, = torch.autograd.grad(loss2, gg)

    e = dict(loss=abs(float(loss.detach()) - ref), grad=relmax(grad.cpu().numpy(), gref.numpy()), ref=ref)
    _record(record_testsuite_property, f'hellinger_shapes/{"x".join(map(str, shape))}/alpha{alpha:g}', e)
    assert grad_target is None
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    assert torch.equal(grad_scaled, grad * 0.37)
    assert ref > 0 and torch.isfinite(gref).all()
    assert e['loss'] <= E_LOSS, e
    assert e['grad'] <= E_GRAD, e
