"""CPU-side checks of SSIM / MS-SSIM (hg_ssim_fwd, hg_ssim_bwd, include/hg_post.h; histogan_amd/post.py ssim / ssim_map /
ms_ssim): the fp64 reference helper of tests/ssim_ref.py against closed-form anchors, an independent scipy evaluation and its own
hand-written gradient, and the host side of the C ABI (exports, version, workspace query, argument validation) and of the
Python surface.  No kernel is launched.

Before the feature the ABI tests fail for want of the symbols and of version 111, and the Python-surface tests for want of
post.ssim, of project's arguments and of reconstruction_loss('SSIM')."""
import ctypes
import types

import numpy as np
import pytest
import torch

import ssim_ref as R


@pytest.fixture(scope='module')
def L():
    from histogan_amd import build
    build.build()
    import histogan_amd._lib as L
    return L


# ---- the reference helper ----------------------------------------------------------------------------------------------
def test_window_is_the_published_gaussian():
    g = R.window()
    assert g.dtype == torch.float64 and g.shape == (11,) and abs(float(g.sum()) - 1.0) < 1e-15
    assert torch.equal(g, g.flip(0)) and abs(float(g[4] / g[5]) - np.exp(-1 / 4.5)) < 1e-15


@pytest.mark.parametrize('a,b', [(0.2, 0.7), (0.0, 1.0), (0.5, 0.5)])
def test_constant_planes(a, b):
    x, y = torch.full((1, 3, 14, 19), a), torch.full((1, 3, 14, 19), b)
    s, cs = R.plane_maps(R.planes(x, 'rgb'), R.planes(y, 'rgb'))
    a64, b64 = float(torch.tensor(a).double()), float(torch.tensor(b).double())
    want = (2 * a64 * b64 + R.C1) / (a64 * a64 + b64 * b64 + R.C1)
    print(f'constant planes {a}, {b}: ssim {float(s.mean()):.15f}, closed form {want:.15f}, cs - 1 up to {float((cs - 1).abs().max()):.1e}')
    assert float((s - want).abs().max()) <= 1e-12 and float((cs - 1).abs().max()) <= 1e-12


@pytest.mark.parametrize('channels', R.CHANNELS)
def test_equal_and_negated_images(channels):
    pred, target = R.seeded_pair(3, (2, 3, 176, 180))
    v, g = R.fwd_bwd(target, target, channels)
    assert float((v - 1).abs().max()) <= 1e-14 and float(g.abs().max()) <= 1e-14
    ms, g = R.fwd_bwd(target, target, channels, kind='ms-ssim')
    assert float((ms - 1).abs().max()) <= 1e-13
    # y = 1 - x: every window's covariance is -variance, the mean cs is negative, MS-SSIM is 0 with gradient 0
    x = target
    if channels == 'rgb':
        _, cs = R.ssim_means(x, 1 - x, channels)
        assert float(cs.max()) < 0
        ms, g = R.fwd_bwd(x, 1 - x, channels, kind='ms-ssim')
        assert float(ms.abs().max()) == 0.0 and float(g.abs().max()) == 0.0 and bool(torch.isfinite(g).all())
    else:                                       # (L* of 1 - x is not 1 - L*; negate the plane's source instead: greys)
        grey = x[:, :1].expand(-1, 3, -1, -1)
        _, cs = R.ssim_means(grey, 1 - grey, channels)
        assert float(cs.max()) < 0
        ms, g = R.fwd_bwd(grey, 1 - grey, channels, kind='ms-ssim')
        assert float(ms.abs().max()) == 0.0 and float(g.abs().max()) == 0.0 and bool(torch.isfinite(g).all())


def test_map_against_scipy():
    from scipy import ndimage, signal
    pred, target = R.seeded_pair(5, (1, 3, 37, 45))
    x, y = R.planes(pred, 'L')[0, 0].numpy(), R.planes(target, 'L')[0, 0].numpy()
    g = R.window().numpy()
    # two independent evaluations of the valid window means: a 2-D convolution with the outer product, and two 1-D
    # correlations cropped to the positions whose window lies inside
    k2 = np.outer(g, g)
    conv = lambda p: signal.convolve2d(p, k2, mode='valid')                                                   # noqa: E731
    corr = lambda p: ndimage.correlate1d(ndimage.correlate1d(p, g, axis=0, mode='constant'), g, axis=1, mode='constant')[5:-5, 5:-5]  # noqa: E731
    ours = R.ssim_map(pred, target, 'L')[0].numpy()
    for name, blur in (('convolve2d', conv), ('correlate1d', corr)):
        mx, my = blur(x), blur(y)
        sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
        want = (2 * mx * my + R.C1) / (mx * mx + my * my + R.C1) * (2 * sxy + R.C2) / (sxx + syy + R.C2)
        err = float(np.abs(ours - want).max())
        print(f'reference map against scipy {name}: {err:.2e} on values up to {float(np.abs(want).max()):.3f}')
        assert ours.shape == want.shape == (27, 35) and err <= 1e-12


@pytest.mark.parametrize('a,c', [((1.0, 1.0), (0.0, 0.0)), ((0.0, 0.0), (1.0, 1.0)), ((0.7, -1.3), (2.1, 0.4))])
@pytest.mark.parametrize('channels', R.CHANNELS)
def test_analytic_gradient_against_autograd(channels, a, c):
    pred, target = R.seeded_pair(6, (2, 3, 23, 29))
    a, c = torch.tensor(a, dtype=torch.float64), torch.tensor(c, dtype=torch.float64)
    x = R.planes(pred, channels).detach().requires_grad_(True)
    y = R.planes(target, channels)
    s, cs = R.plane_means(x, y)
    want, = torch.autograd.grad((a * s + c * cs).sum(), x)
    got = R.analytic_plane_grad(x.detach(), y, a, c)
    err = float((got - want).abs().max() / want.abs().max())
    print(f'three-map gradient against autograd ({channels}, a={a.tolist()}, c={c.tolist()}): {err:.2e} of {float(want.abs().max()):.2e}')
    assert err <= 1e-12


def test_ms_ssim_levels_reach_the_window_at_176():
    pred, target = R.seeded_pair(7, (1, 3, 176, 176))
    lv = R.ms_ssim_levels(pred, target)
    assert [s for _, _, s in lv] == [(176, 176), (88, 88), (44, 44), (22, 22), (11, 11)]
    lv = R.ms_ssim_levels(*R.seeded_pair(7, (1, 3, 183, 201)))
    assert [s for _, _, s in lv] == [(183, 201), (91, 100), (45, 50), (22, 25), (11, 12)]
    assert abs(sum(R.WEIGHTS) - 1.0001) < 1e-12


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def test_symbols_version_and_constants(L):
    from histogan_amd import post
    for name in ('hg_ssim_fwd', 'hg_ssim_bwd', 'hg_ssim_workspace_bytes', 'hg_ssim_tile', 'hg_ssim_finish_threads'):
        assert name in L.EXPORTS and hasattr(L.lib, name)
    assert L.lib.hg_version() >= 111
    assert post.SSIM_TILE == L.lib.hg_ssim_tile() and post.SSIM_FINISH_THREADS == L.lib.hg_ssim_finish_threads()
    assert post.MS_SSIM_WEIGHTS == R.WEIGHTS and post.MS_SSIM_MIN_SIZE == 176 and post.SSIM_WINDOW == R.TAPS


def test_workspace_query(L):
    from histogan_amd import post
    q, T = L.lib.hg_ssim_workspace_bytes, post.SSIM_TILE
    assert q(1, 11, 11) == 16                                                  # one tile: (sum ssim, sum cs), fp64
    assert q(1, T + 10, T + 10) == 16 and q(1, T + 11, T + 10) == 32 and q(1, T + 11, 2 * T + 13) == 6 * 16
    assert q(3, T + 11, 2 * T + 13) == 3 * 6 * 16
    assert q(0, 64, 64) == 0 and q(1, 10, 64) == 0 and q(1, 64, 10) == 0 and q(1, 64, -1) == 0 and q(65536, 64, 64) == 0


def test_bad_arguments_are_refused_before_any_launch(L):
    """The library loads without a GPU; every call below returns HG_EINVAL (-1) before it would launch, so the pointers --
    never dereferenced on the host -- need not be real."""
    p = ctypes.c_void_p(4096)
    B, H, W = 2, 40, 50
    ws = L.lib.hg_ssim_workspace_bytes(B, H, W)
    s = (3 * H * W, H * W, W, 1)
    EINVAL = -1

    def fwd(x1=p, x2=p, mode=0, means=p, smap=None, pool1=None, pool2=None, B=B, H=H, W=W, workspace=p, nbytes=ws):
        return L.lib.hg_ssim_fwd(x1, *s, x2, *s, mode, means, smap, pool1, pool2, B, H, W, workspace, nbytes, None)

    def bwd(x1=p, x2=p, mode=0, coef=p, coarse=None, grad=p, B=B, H=H, W=W):
        return L.lib.hg_ssim_bwd(x1, *s, x2, *s, mode, coef, coarse, grad, B, H, W, None)

    assert fwd(x1=None) == EINVAL and fwd(x2=None) == EINVAL and fwd(means=None) == EINVAL and fwd(workspace=None) == EINVAL
    assert fwd(pool1=p) == EINVAL and fwd(pool2=p) == EINVAL                   # both or neither
    assert fwd(H=10) == EINVAL and fwd(W=10) == EINVAL and fwd(H=0) == EINVAL and fwd(W=-3) == EINVAL
    assert fwd(B=0) == EINVAL and fwd(B=-1) == EINVAL and fwd(B=65536, nbytes=1 << 40) == EINVAL
    assert fwd(mode=4) == EINVAL and fwd(mode=-1) == EINVAL
    assert fwd(nbytes=ws - 1) == EINVAL and fwd(nbytes=0) == EINVAL and fwd(smap=p, pool1=p, pool2=p, nbytes=ws - 1) == EINVAL
    assert bwd(x1=None) == EINVAL and bwd(x2=None) == EINVAL and bwd(coef=None) == EINVAL and bwd(grad=None) == EINVAL
    assert bwd(H=10) == EINVAL and bwd(W=10) == EINVAL and bwd(B=0) == EINVAL and bwd(B=65536) == EINVAL
    assert bwd(mode=4) == EINVAL and bwd(mode=-1) == EINVAL and bwd(coarse=p, mode=7) == EINVAL


# ---- the Python surface refuses before a device is touched ----------------------------------------------------------------
@pytest.mark.parametrize('channels', ['l', 'RGB', 'lab', None, 0, True])
def test_bad_channels_raise_value_error(L, channels):
    from histogan_amd import post
    x = torch.rand(1, 3, 176, 176)
    for fn in (post.ssim, post.ssim_map, post.ms_ssim):
        with pytest.raises(ValueError, match="'L'.*'rgb'"):
            fn(x, x, channels=channels)


def test_bad_shapes_sizes_and_devices(L):
    from histogan_amd import post
    x = torch.rand(2, 3, 32, 32)
    for fn in (post.ssim, post.ssim_map, post.ms_ssim):
        with pytest.raises(ValueError, match=r'\(B, 3, H, W\)'):
            fn(torch.rand(2, 1, 32, 32), torch.rand(2, 1, 32, 32))
        with pytest.raises(ValueError, match=r'\(B, 3, H, W\)'):
            fn(torch.rand(32, 32), torch.rand(32, 32))
        with pytest.raises(ValueError, match=r'\(B, 3, H, W\)'):
            fn(x.to(torch.int32), x)
        with pytest.raises(ValueError, match='one shape and device'):
            fn(x, torch.rand(2, 3, 32, 33))
        with pytest.raises(ValueError, match='one shape and device'):
            fn(x, x.to('meta'))
    with pytest.raises(ValueError, match='at least 11 x 11'):
        post.ssim(torch.rand(1, 3, 10, 40), torch.rand(1, 3, 10, 40))
    with pytest.raises(ValueError, match='at least 11 x 11'):
        post.ssim_map(torch.rand(3, 40, 10), torch.rand(3, 40, 10))
    with pytest.raises(ValueError, match='at least 176 x 176'):
        post.ms_ssim(torch.rand(1, 3, 175, 300), torch.rand(1, 3, 175, 300))
    # sizes that pass: the refusal left is the device's, as everywhere in post
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        post.ssim(x, x)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        post.ms_ssim(torch.rand(1, 3, 176, 176), torch.rand(1, 3, 176, 176), channels='rgb')


def test_project_and_reconstruction_loss_refusals(L):
    from histogan_amd import project
    from histogan_amd.retrainer import reconstruction_loss
    for kind in ('SSIM', 'msssim', None, 5):
        with pytest.raises(ValueError, match="'ssim' or 'ms-ssim'"):
            project.project(None, None, ssim_weight=1.0, ssim_kind=kind)
    small = types.SimpleNamespace(GE=types.SimpleNamespace(image_size=128))
    with pytest.raises(ValueError, match='image_size >= 176'):
        project.project(small, None, ssim_weight=0.5, ssim_kind='ms-ssim')
    # the reconstruction loss goes through post.ssim and inherits its refusals
    f = reconstruction_loss('SSIM')
    with pytest.raises(ValueError, match='at least 11 x 11'):
        f.compute_loss(torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8))
    with pytest.raises(ValueError, match='one shape and device'):
        f.compute_loss(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 20))
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        f.compute_loss(torch.rand(1, 4, 16, 16), torch.rand(1, 4, 16, 16))         # (the first three channels are taken)
