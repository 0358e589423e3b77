"""CPU-side checks of the CIE colour difference (hg_delta_e, include/hg_post.h; histogan_amd/post.py delta_e / delta_e_map):
the fp64 reference helper of tests/delta_e_ref.py against the published CIEDE2000 test pairs and the properties of a
distance, and the host side of the C ABI (exports, version, workspace query, argument validation).  No kernel is launched.

Before the feature the ABI tests fail for want of the symbols and of version 110, and the Python-surface tests for want of
post.delta_e and of project's arguments."""
import ctypes

import pytest
import torch

import delta_e_ref as R
import lab_ref


@pytest.fixture(scope='module')
def L():
    from histogan_amd import build
    build.build()
    import histogan_amd._lib as L
    return L


# ---- the reference helper ----------------------------------------------------------------------------------------------
def test_helper_reproduces_the_published_pairs():
    worst = R.check_sharma()
    print(f'dE00 helper against the {len(R.SHARMA)} published pairs: largest deviation {worst:.2e}')
    assert len(R.SHARMA) == 25 and worst <= R.SHARMA_TOL
    # the pairs on both sides of the hue branches differ as published (not merely each within the bar)
    de = R.delta_e_lab(torch.tensor([p[0] for p in R.SHARMA], dtype=torch.float64),
                       torch.tensor([p[1] for p in R.SHARMA], dtype=torch.float64), 2000)
    assert float(de[10] - de[9]) > 0.03 and float(de[13] - de[14]) > 0.05


@pytest.mark.parametrize('kind', R.KINDS)
def test_helper_is_a_symmetric_distance_with_a_finite_gradient(kind):
    pred, target = R.seeded_pair(12, (2, 3, 16, 24))
    a, b = R.delta_e_map(pred, target, kind), R.delta_e_map(target, pred, kind)
    sym = float((a - b).abs().max())
    print(f'dE{kind}: asymmetry {sym:.2e} on values up to {float(a.max()):.1f}')
    assert sym <= 1e-12 * float(a.max()) and float(a.min()) > 0
    for x in (pred, lab_ref.edge_image()):                      # equal inputs, the edge pixels included
        m, mean, g = R.fwd_bwd(x, x, kind)
        assert float(m.abs().max()) == 0.0 and float(mean.abs().max()) == 0.0
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) == 0.0
    # the edge pixels against a shifted copy: singular pixels (black, white, grey), finite gradient, zero where clamped
    e = lab_ref.edge_image()
    m, mean, g = R.fwd_bwd(e, e.roll(1, 3), kind)
    assert bool(torch.isfinite(m).all()) and bool(torch.isfinite(g).all())
    assert bool((g[(e < 0) | (e > 1)] == 0).all())


def test_weighted_mean_of_the_helper():
    pred, target = R.seeded_pair(11, (2, 3, 7, 5))
    ones = torch.ones(2, 7, 5)
    assert torch.equal(R.delta_e_mean(pred, target, 2000, ones), R.delta_e_mean(pred, target, 2000))
    assert float(R.delta_e_mean(pred, target, 2000, 0 * ones).abs().max()) == 0.0
    m, mean, g = R.fwd_bwd(pred, target, 2000, weight=0 * ones)
    assert float(g.abs().max()) == 0.0 and bool(torch.isfinite(g).all())


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def test_symbols_and_version(L):
    assert 'hg_delta_e' in L.EXPORTS and 'hg_delta_e_workspace_bytes' in L.EXPORTS
    assert hasattr(L.lib, 'hg_delta_e') and hasattr(L.lib, 'hg_delta_e_workspace_bytes')
    assert L.lib.hg_version() >= 110


def test_workspace_query(L):
    q = L.lib.hg_delta_e_workspace_bytes
    assert q(1, 1, 1) > 0
    sizes = [(1, 1), (16, 16), (16, 17), (33, 40), (256, 256), (300, 300), (1024, 1024)]
    for B in (1, 2, 32):
        got = [q(B, h, w) for h, w in sizes]
        assert all(g > 0 for g in got) and got == sorted(got), got
        assert all(q(B + 1, h, w) >= q(B, h, w) for h, w in sizes)
    assert q(2, 256, 256) > q(1, 256, 256) and q(1, 300, 300) > q(1, 16, 16)
    assert q(0, 4, 4) == 0 and q(1, 0, 4) == 0 and q(1, 4, -1) == 0        # refused sizes have no workspace


def test_bad_arguments_are_refused_before_any_launch(L):
    """The library loads without a GPU; every call below returns HG_EINVAL (-1) before it would launch, so the pointers --
    never dereferenced on the host -- need not be real."""
    p = ctypes.c_void_p(4096)
    B, H, W = 2, 8, 8
    ws = L.lib.hg_delta_e_workspace_bytes(B, H, W)
    s = (3 * H * W, H * W, W, 1)
    wstr = (H * W, W, 1)

    def call(x1=p, x2=p, weight=None, kind=2000, mean=p, dmap=None, grad=None, B=B, H=H, W=W, workspace=p, nbytes=ws):
        return L.lib.hg_delta_e(x1, *s, x2, *s, weight, *wstr, kind, mean, dmap, grad, B, H, W, workspace, nbytes, None)

    EINVAL = -1
    assert call(x1=None) == EINVAL and call(x2=None) == EINVAL and call(mean=None) == EINVAL
    assert call(workspace=None) == EINVAL
    assert call(B=0) == EINVAL and call(H=0) == EINVAL and call(W=0) == EINVAL and call(B=-1) == EINVAL
    assert call(kind=94) == EINVAL and call(kind=0) == EINVAL
    assert call(nbytes=ws - 1) == EINVAL and call(nbytes=0) == EINVAL
    assert call(B=65536, nbytes=1 << 40) == EINVAL                         # beyond the grid's y extent
    assert call(weight=p, grad=p, dmap=p, nbytes=ws - 1) == EINVAL


# ---- the Python surface refuses before a device is touched ----------------------------------------------------------------
@pytest.mark.parametrize('kind', ['94', 94, 'ciede2000', None, 2000.5, True])
def test_bad_kind_raises_value_error(L, kind):
    from histogan_amd import post, project
    x = torch.rand(1, 3, 4, 4)
    with pytest.raises(ValueError, match="'76' or '2000'"):
        post.delta_e(x, x, kind=kind)
    with pytest.raises(ValueError, match="'76' or '2000'"):
        post.delta_e_map(x, x, kind=kind)
    with pytest.raises(ValueError, match="'76' or '2000'"):
        project.project(None, None, delta_e_weight=1.0, delta_e_kind=kind)


def test_good_kinds_and_the_other_refusals(L):
    from histogan_amd import post
    assert [post.delta_e_kind(k) for k in ('76', '2000', 76, 2000)] == [76, 2000, 76, 2000]
    x = torch.rand(1, 3, 4, 4)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        post.delta_e(x, x)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        post.delta_e_map(x, x, kind='76')
    with pytest.raises(ValueError, match='weight'):
        post.delta_e(x, x, weight=torch.rand(1, 4, 4, requires_grad=True))
