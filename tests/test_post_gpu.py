"""The full-resolution post-processing kernels (include/hg_post.h) through histogan_amd/post.py, the drop-ins at the
reference's import paths (utils/imresize.py, utils/pyramid_upsampling.py, utils/color_transfer_MKL.py) and
recoloringTrainer.evaluate's 'upscaling'/'pyramid' and post_recoloring branches, against the reference-derived fixtures
(tests/golden/post_*.npz) and, at the sizes a user runs, against the fp64 restatement tests/post_ref.py.

Bars: float images max abs <= 1e-5 on [0, 1] data; T relative <= 1e-6; uint8 equal except <= 1 LSB where the fp64 value
lies within 5e-3 (0-255 units) of a rounding boundary."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)


@pytest.fixture(scope='module')
def P():
    from histogan_amd import build
    build.build()
    from histogan_amd import post
    return post


@pytest.fixture(scope='module')
def R(P):
    import post_ref
    return post_ref


def _cases(fname):
    z = np.load(os.path.join(GOLDEN_DIR, fname))
    out = {}
    for k in z.files:
        name, _, field = k.partition('/')
        out.setdefault(name, {})[field] = z[k]
    return out


IMRESIZE = _cases('post_imresize.npz')
MKLC = _cases('post_mkl.npz')
PYR = sorted(glob.glob(os.path.join(GOLDEN_DIR, 'post_pyr_*.npz')))


def maxabs(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)))


def check_u8(got, want, allowed):
    """got == want except <= 1 LSB where `allowed` (near a rounding boundary)."""
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1, d.max()
    assert np.all(allowed[d == 1]), f'{int((d == 1).sum())} off-by-one outputs, not all at a rounding boundary'


def near_trunc(v, tol=5e-3):
    """fp64 values v (0-255 units) truncated to uint8: within tol of an integer."""
    return np.abs(v - np.round(v)) < tol


def photo(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W] / max(H, W)
    ch = [0.5 + 0.3 * np.sin(2 * np.pi * rng.uniform(1, 6) * yy + rng.uniform(0, 6)) *
          np.cos(2 * np.pi * rng.uniform(1, 6) * xx + rng.uniform(0, 6)) for _ in range(3)]
    img = np.stack(ch, -1) + rng.normal(0, 0.06, (H, W, 3))
    return np.clip(np.round(img * 255), 0, 255).astype(np.uint8)


# ---- imresize ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(IMRESIZE))
def test_imresize_dropin_matches_fixture(P, R, name):
    import utils.imresize as U
    c = IMRESIZE[name]
    kw = json.loads(str(c['kwargs']))
    x = c['x'].copy()
    out = U.imresize(x, **kw)
    np.testing.assert_array_equal(x, c['x'])                                    # input untouched
    if c['out'].dtype == np.uint8:
        assert out.dtype == np.uint8
        _, raw, tabs = R.imresize(c['x'], with_raw=True, **kw)
        check_u8(out, c['out'], R.u8_near_boundary(raw, tabs))
    else:
        assert out.dtype == np.float64
        assert maxabs(out, c['out']) <= 1e-5


def test_imresize_device_layouts(P, R):
    rng = np.random.default_rng(1)
    x = rng.random((3, 75, 101)).astype(np.float32)
    xt = torch.from_numpy(x).to(DEV)
    out = P.imresize(xt, output_shape=(150, 202)).cpu().numpy()
    ref = R.imresize(x.transpose(1, 2, 0), output_shape=(150, 202)).transpose(2, 0, 1)
    assert maxabs(out, ref) <= 1e-5
    hwc = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 2, 0))).to(DEV).permute(2, 0, 1)   # strided view
    assert torch.equal(P.imresize(hwc, output_shape=(150, 202)).cpu(), torch.from_numpy(out))
    with pytest.raises(ValueError):
        P.imresize(xt, output_shape=(10, 10), method='lanczos')


# ---- pyramid ----------------------------------------------------------------------------------------------------------
def _pyr_inputs(z):
    ref = z['reference_u8'].transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    return z['target'], ref


@pytest.mark.parametrize('path', PYR, ids=[os.path.basename(p)[9:-4] for p in PYR])
def test_pyramid_matches_fixture(P, path):
    import utils.pyramid_upsampling as U
    z = np.load(path)
    kw = json.loads(str(z['kwargs']))
    target, ref = _pyr_inputs(z)
    tt = torch.from_numpy(target.copy()).unsqueeze(0)
    out = U.pyramid_upsampling(tt, torch.from_numpy(ref).unsqueeze(0), **kw)      # CPU tensors in, as the reference
    assert out.dtype == torch.float64 and out.device.type == 'cpu'
    assert maxabs(out[0].numpy(), z['out']) <= 1e-5
    assert np.array_equal(tt[0].numpy(), target)                                  # the caller's target is not clamped
    # the device API with the uint8 reference, as evaluate uploads it
    o2 = P.pyramid_upsampling(torch.from_numpy(target).to(DEV), torch.from_numpy(z['reference_u8']).to(DEV), **kw)
    assert maxabs(o2[0].cpu().numpy(), z['out']) <= 1e-5


@pytest.mark.parametrize('H,W,levels', [(1536, 1152, 6), (1500, 1000, 6)])
def test_pyramid_user_size_vs_post_ref(P, R, H, W, levels):
    rng = np.random.default_rng(H + W)
    ref_u8 = photo(rng, H, W)
    target = (rng.random((3, 256, 256)) * 1.2 - 0.1).astype(np.float32)
    tdev, rdev = torch.from_numpy(target).to(DEV), torch.from_numpy(ref_u8).to(DEV)
    out = P.pyramid_upsampling(tdev, rdev, levels=levels, swapping_levels=1)
    want = R.pyramid_upsampling(target, ref_u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255), levels, 1)
    assert out.shape[2:] == P.padded_size(H, W, levels)
    assert maxabs(out[0].cpu().numpy(), want) <= 1e-5
    again = P.pyramid_upsampling(tdev, rdev, levels=levels, swapping_levels=1)
    assert torch.equal(out, again)                                                # bit-identical repeats
    assert np.array_equal(tdev.cpu().numpy(), target) and np.array_equal(rdev.cpu().numpy(), ref_u8)
    u8 = P.float_to_u8_hwc(out[0]).cpu().numpy()
    v = np.clip(want, 0, 1).transpose(1, 2, 0) * 255 + 0.5
    check_u8(u8, R.save_image_u8(want), near_trunc(v))


@pytest.mark.parametrize('H,W', [(75, 51), (37, 90), (1, 7), (6, 1), (2, 3), (129, 257)])
def test_pyr_kernels_odd_sizes_every_level(P, R, H, W):
    rng = np.random.default_rng(H * 1000 + W)
    x = rng.random((3, H, W)).astype(np.float32)
    cur, ref = torch.from_numpy(x).to(DEV), x.transpose(1, 2, 0).astype(np.float64)
    while True:                                    # pyrDown down to 1x1, every level odd or even as it falls
        assert maxabs(cur.cpu().numpy().transpose(1, 2, 0), ref) <= 1e-5
        up = P.pyr_up_add(cur)                     # plain pyrUp of every level
        assert maxabs(up.cpu().numpy().transpose(1, 2, 0), R.pyrUp(ref)) <= 1e-5
        if cur.shape[1] == 1 and cur.shape[2] == 1:
            break
        cur, ref = P.pyr_down(cur), R.pyrDown(ref)
    # the fused add: pyrUp(prev) + wa (fine_a - pyrUp(coarse_a)) + wb (fine_b - pyrUp(coarse_b)), odd source sizes
    h, w = (H + 1) // 2, (W + 1) // 2
    prev, ca, cb = (rng.random((3, h, w)).astype(np.float32) for _ in range(3))
    fa, fb = (rng.random((3, 2 * h, 2 * w)).astype(np.float32) for _ in range(2))
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    got = P.pyr_up_add(t(prev), t(fa), t(ca), 0.25, t(fb), t(cb), 0.75).cpu().numpy()
    U = lambda a: R.pyrUp(a.transpose(1, 2, 0).astype(np.float64)).transpose(2, 0, 1)  # noqa: E731
    assert maxabs(got, U(prev) + 0.25 * (fa - U(ca)) + 0.75 * (fb - U(cb))) <= 1e-5


def test_pyramid_errors(P):
    t = torch.rand(1, 3, 64, 64, device=DEV)
    r = torch.rand(1, 3, 128, 96, device=DEV)
    with pytest.raises(IndexError):
        P.pyramid_upsampling(t, r, levels=5, swapping_levels=2, blending=True)
    with pytest.raises(IndexError):
        P.pyramid_upsampling(t, r, levels=3, swapping_levels=4)
    with pytest.raises(ValueError):
        P.pyramid_upsampling(t, torch.rand(1, 4, 128, 96, device=DEV), levels=3)
    with pytest.raises(ValueError):
        P.pyramid_upsampling(torch.rand(1, 1, 64, 64, device=DEV), r, levels=3)
    with pytest.raises(ValueError):
        P.pyramid_upsampling(t, torch.zeros(128, 96, 4, dtype=torch.uint8, device=DEV), levels=3)


# ---- colour transfer --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(MKLC))
def test_mkl_matches_fixture(P, R, name):
    import utils.color_transfer_MKL as U
    c = MKLC[name]
    out = U.color_transfer_MKL(c['source'], c['target'])
    assert out.dtype == np.float64 and out.shape == c['source'].shape
    o2, T = P.color_transfer_mkl(torch.from_numpy(c['source']).to(DEV), torch.from_numpy(c['target']).to(DEV))
    m, cov = P.color_moments(torch.from_numpy(c['source']).to(DEV))
    np.testing.assert_allclose(cov, c['A'], rtol=1e-9, atol=1e-12)
    # T is defined by the reference only up to LAPACK's eigenvector signs (see post_ref.mkl_sign_variants): it must be
    # the fixture's T, or one of its sign variants, to 1e-6; the image must be that T's affine map to 1e-5
    variants = R.mkl_sign_variants(c['A'], c['B'])
    rels = [np.max(np.abs(T - v)) / np.max(np.abs(v)) for v in variants]
    k = int(np.argmin(rels))
    assert rels[k] <= 1e-6, (min(rels), np.max(np.abs(T - c['T'])) / np.max(np.abs(c['T'])))
    x = c['source'].reshape(-1, 3).astype(np.float64)
    y = c['target'].reshape(-1, 3).astype(np.float64)
    want = np.clip((x - x.mean(0)) @ variants[k] + y.mean(0), 0, 1).reshape(c['source'].shape)
    assert maxabs(out, want) <= 1e-5
    if np.max(np.abs(variants[k] - c['T'])) <= 1e-6 * np.max(np.abs(c['T'])):
        assert maxabs(out, c['out']) <= 1e-5
    assert torch.equal(o2, P.color_transfer_mkl(torch.from_numpy(c['source']).to(DEV),
                                                torch.from_numpy(c['target']).to(DEV))[0])      # bit-identical
    assert U.EPS == 2.2204e-16 and callable(U.MKL)


def test_mkl_user_size_vs_post_ref(P, R):
    rng = np.random.default_rng(7)
    src = (photo(rng, 1512, 2016) / 255).astype(np.float32)
    gen = (rng.random((3, 256, 256)) * 1.3 - 0.15).astype(np.float32)                 # unclamped network output
    sd, gd = torch.from_numpy(src).to(DEV), torch.from_numpy(gen).to(DEV)
    out, T = P.color_transfer_mkl(sd, gd.permute(1, 2, 0))
    want, Tw = R.color_transfer(src, gen.transpose(1, 2, 0))
    assert np.max(np.abs(T - Tw)) / np.max(np.abs(Tw)) <= 1e-6
    assert maxabs(out.cpu().numpy(), want) <= 1e-5
    u8, _ = P.color_transfer_mkl(sd, gd.permute(1, 2, 0), quantize=True)
    check_u8(u8.cpu().numpy(), (want * 255).astype(np.uint8), near_trunc(want * 255))
    assert np.array_equal(sd.cpu().numpy(), src) and np.array_equal(gd.cpu().numpy(), gen)
    with pytest.raises(ValueError):
        P.color_transfer_mkl(torch.rand(10, 10, 4, device=DEV), gd.permute(1, 2, 0))


# ---- recoloringTrainer.evaluate ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def trainer(P, tmp_path_factory):
    torch.manual_seed(0)
    from ReHistoGAN.rehistoGAN import recoloringTrainer
    d = tmp_path_factory.mktemp('evalpost')
    tr = recoloringTrainer('post', str(d / 'results'), str(d / 'models'), image_size=64, network_capacity=4,
                           batch_size=1, hist_bin=16, hist_insz=32)
    tr.init_GAN()
    return tr, d


@pytest.mark.parametrize('mode', ['pyramid', 'mkl', 'both'])
def test_evaluate_full_resolution(P, R, trainer, monkeypatch, mode):
    from PIL import Image
    tr, d = trainer
    rng = np.random.default_rng(3)
    photo_u8 = photo(rng, 200, 300)                                    # a 300x200 (W x H) photo
    name = str(d / f'photo_{mode}.png')
    Image.fromarray(photo_u8).save(name)
    original_img = np.array(Image.open(name)) / 255                     # rehistoGAN.py:77-79
    img = torch.rand(1, 3, 64, 64, device=DEV)
    h = torch.rand(1, 3, 16, 16, device=DEV)
    h = h / h.sum(dim=(1, 2, 3), keepdim=True)
    writes = []
    real = P.save_rgb
    monkeypatch.setattr(P, 'save_rgb', lambda a, p: (writes.append((a.cpu().numpy().copy(), p)), real(a, p)))
    up, rec = mode in ('pyramid', 'both'), mode in ('mkl', 'both')
    with torch.no_grad():
        g = tr.evaluate(f'out_{mode}', image_batch=img, hist_batch=h, resizing='upscaling' if up else None,
                        resizing_method='pyramid', swapping_levels=1, pyramid_levels=5, level_blending=False,
                        original_size=[300, 200], original_image=original_img, input_image_name=name,
                        save_input=False, post_recoloring=rec)
    gen = g[0].cpu().numpy().astype(np.float32)
    out_name = str(d / 'results' / 'post' / f'out_{mode}-generated.jpg')
    assert [p for _, p in writes] == [out_name] * (int(up) + int(rec))
    i = 0
    if up:
        want = R.pyramid_upsampling(gen, photo_u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255), 5, 1)
        v = np.clip(want, 0, 1).transpose(1, 2, 0) * 255 + 0.5
        assert writes[0][0].shape == (224, 320, 3)                     # padded to multiples of 2**5, kept
        check_u8(writes[0][0], R.save_image_u8(want), near_trunc(v))
        i = 1
    if rec:
        want, _ = R.color_transfer(original_img, gen.transpose(1, 2, 0))
        check_u8(writes[i][0], (want * 255).astype(np.uint8), near_trunc(want * 255))
    with Image.open(out_name) as im:
        assert im.size == ((300, 200) if rec else (320, 224))


def test_evaluate_errors(trainer):
    tr, d = trainer
    img = torch.rand(2, 3, 64, 64, device=DEV)
    h = torch.rand(2, 3, 16, 16, device=DEV)
    with torch.no_grad():
        with pytest.raises(ValueError):
            tr.evaluate('e1', image_batch=img, hist_batch=h, post_recoloring=True, original_image=np.zeros((4, 4, 3)),
                        save_input=False)
        with pytest.raises(NotImplementedError):
            tr.evaluate('e2', image_batch=img[:1], hist_batch=h[:1], resizing='upscaling', resizing_method='BGU',
                        save_input=False)
