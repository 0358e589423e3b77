"""The discriminator phase both trainers share (histogan_amd/trainer.py::discriminator_phase) on a stub discriminator, plain
torch on the CPU: one pass over [fake; real] against two passes, the autograd route, and what the augment callable sees.

The stub follows `Discriminator.forward`'s contract: (scores (N,), quantize loss (1,)).  Its quantize loss is a sum of
per-sample terms: a per-sample VECTOR would be averaged over B samples by the two-pass branch and over 2 B by the one-pass
branch, which no trainer ever does (feature quantisation always takes two passes).  Inputs, weights and the per-sample
terms are small dyadic fractions, so every sum is exact in fp32 whatever order a convolution or a reduction takes."""
import torch
import torch.nn.functional as F

from histogan_amd import trainer as T

B = 2


class StubDisc(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(1)
        self.weight = torch.nn.Parameter(torch.randint(-4, 5, (1, 3, 8, 8), generator=g) / 4.0)

    def forward(self, x):
        per_sample = (x.detach()[:, 0, 0, 0] * 8).round() / 8        # quantize-loss term of each sample
        return F.conv2d(x, self.weight).squeeze(), per_sample.sum().reshape(1)


def _batches(seed=0):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randint(-8, 9, (B, 3, 8, 8), generator=g) / 8.0 for _ in range(2))


def test_one_pass_equals_two_passes():
    D = StubDisc()
    fake, real = _batches()
    real1, div1, q1 = T.discriminator_phase(D, fake, real, B, False)
    real2, div2, q2 = T.discriminator_phase(D, fake, real, B, True)
    assert float(q2) != 0.0 and float(div2) > 0.0                  # (the case is not degenerate)
    assert torch.equal(div1, div2) and torch.equal(q1, q2) and torch.equal(real1, real2)
    assert torch.equal(real2, D(real)[0])
    want = (F.relu(1 + D(real)[0]) + F.relu(1 - D(fake)[0])).mean()
    assert torch.equal(div2, want)


def test_batch_with_a_graph_goes_through_cat(monkeypatch):
    D = StubDisc()
    fake, real = _batches(1)
    calls = []
    real_cat = torch.cat
    monkeypatch.setattr(torch, 'cat', lambda *a, **k: calls.append(1) or real_cat(*a, **k))
    T.discriminator_phase(D, fake, real, B, False)
    assert not calls                                               # no graph: the two-copy concatenation
    real.requires_grad_(True)
    real_output, div, _ = T.discriminator_phase(D, fake, real, B, False)
    assert calls == [1] and real_output.requires_grad
    div.backward()
    # d mean(relu(1 + D(real_i)) + ...) / d real_i = weight / B where the hinge is active, 0 elsewhere
    active = (1 + real_output.detach() > 0).float().view(B, 1, 1, 1)
    assert real.grad is not None and torch.equal(real.grad, active * D.weight.detach() / B)
    assert float(active.sum()) > 0


def test_augment_sees_fake_detached_and_real_not():
    D = StubDisc()
    fake, real = _batches(2)
    for two_passes in (False, True):
        seen = []

        def augment(images, detach=False):
            seen.append((images, detach))
            return images + 1          # (what the discriminator scores is the augmented batch)
        real_output, div, q = T.discriminator_phase(D, fake, real, B, two_passes, augment)
        assert len(seen) == 2 and seen[0][0] is fake and seen[0][1] is True and seen[1][0] is real and seen[1][1] is False
        assert torch.equal(real_output, D(real + 1)[0])
        assert torch.equal(div, T.discriminator_phase(D, fake + 1, real + 1, B, two_passes)[1])
