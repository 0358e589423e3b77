"""Host-side checks of the noise-image gradient and the projection driver (no device): the hg_noise_grad export and its
argument guards (include/hg_nets.h), the version-keyed cache of the transposed noise image (nets._noise_t) and
project()'s refusal of the VGG term."""
import os

import pytest
import torch

from conftest import ROOT


@pytest.fixture(scope='module')
def L():
    import histogan_amd._lib as L
    return L


def test_noise_grad_is_exported_and_declared(L):
    assert L.lib.hg_version() >= 109
    assert 'hg_noise_grad' in L.EXPORTS and hasattr(L.lib, 'hg_noise_grad')
    with open(os.path.join(ROOT, 'include', 'hg_nets.h')) as f:
        assert 'int hg_noise_grad(' in f.read()
    from histogan_amd import launch
    assert callable(launch.noise_grad)


def test_noise_grad_refuses_bad_arguments_without_a_device(L):
    f = L.lib.hg_noise_grad
    p = 4096      # (never dereferenced: every call below is refused before a launch)
    assert f(None, None, None, None, 1, 1, 4, 4, 0, None) == -1            # HG_EINVAL
    assert f(None, p, p, p, 1, 1, 4, 4, 0, None) == -1
    assert f(p, p, None, p, 1, 1, 4, 4, 0, None) == -1
    assert f(p, p, p, None, 1, 1, 4, 4, 1, None) == -1
    for B, O, H, S in [(0, 1, 4, 4), (1, 0, 4, 4), (1, 1, 0, 4), (1, 1, -4, 4), (-1, 1, 4, 4)]:
        assert f(p, p, p, p, B, O, H, S, 0, None) == -1
    assert f(p, None, p, p, 1, 1, 8, 4, 0, None) in (-1, -2)               # H > S: as hg_demod_noise_lrelu_fwd
    assert f(p, None, p, p, 1, 1, 8, 4, 0, None) == L.lib.hg_demod_noise_lrelu_fwd(p, None, p, p, p, p, 1, 1, 8, 4, None)


def test_noise_t_cache_follows_in_place_updates():
    from histogan_amd.nets import _noise_t
    t = torch.rand(2, 6, 6, 1)
    a = _noise_t(t)
    assert a.shape == (2, 6, 6) and torch.equal(a, t[..., 0].transpose(1, 2))
    assert _noise_t(t) is a                                  # cached on the tensor
    t.add_(1)                                                # what an optimiser does: the cache must not survive it
    b = _noise_t(t)
    assert b is not a and torch.equal(b, t[..., 0].transpose(1, 2))
    assert _noise_t(t) is b
    with torch.no_grad():
        t.mul_(0.5)
    assert torch.equal(_noise_t(t), t[..., 0].transpose(1, 2))


def test_noise_t_of_a_variable_stays_in_the_graph():
    from histogan_amd.nets import _noise_t
    t = torch.rand(1, 4, 4, 1, requires_grad=True)
    a = _noise_t(t)
    assert a.grad_fn is not None and a.requires_grad
    assert _noise_t(t) is not a and not hasattr(t, '_hg_nzt')      # not cached
    g = torch.rand(1, 4, 4)
    a.backward(g)
    assert torch.equal(t.grad, g.transpose(1, 2)[..., None])        # autograd transposes the gradient back
    # a tensor cached while it was constant and made a variable afterwards leaves the cache behind
    u = torch.rand(1, 4, 4, 1)
    c = _noise_t(u)
    u.requires_grad_()
    assert _noise_t(u) is not c and _noise_t(u).grad_fn is not None


def test_project_refuses_the_vgg_term_before_touching_a_device():
    from histogan_amd import project
    with pytest.raises(NotImplementedError, match='VGG16'):
        project.project(None, None, steps=1, lr=0.1, vgg_loss_weight=0.1)
    with pytest.raises(ValueError):
        project.project(None, None, steps=1, lr=0.1, pixel_loss='L3')
