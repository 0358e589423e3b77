"""CPU-side checks of the full-resolution post-processing (histogan_amd/post.py, include/hg_post.h): the fp64 restatement
tests/post_ref.py reproduces the reference-derived fixtures (tests/golden/post_*.npz, tests/golden/make_golden_post.py),
the host-built resize tables equal the reference's, and the C ABI rejects bad arguments without launching anything."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR


@pytest.fixture(scope='module')
def L():
    from histogan_amd import build
    build.build()
    import histogan_amd._lib as L
    return L


@pytest.fixture(scope='module')
def R(L):
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


@pytest.mark.parametrize('name', sorted(IMRESIZE))
def test_contributions_tables_match_reference(L, name):
    from histogan_amd import post
    c = IMRESIZE[name]
    kw = json.loads(str(c['kwargs']))
    (Ho, Wo), scale = post.resize_plan(c['x'].shape[:2], kw.get('output_shape'), kw.get('scalar_scale'))
    for k, tag, n_out in ((0, 'h', Ho), (1, 'w', Wo)):
        w, i = post.contributions(c['x'].shape[k], n_out, scale[k], post.KERNELS[kw.get('method', 'bicubic')],
                                  post.KERNEL_WIDTH)
        np.testing.assert_array_equal(i, c['i' + tag])
        np.testing.assert_array_equal(w, c['w' + tag])


@pytest.mark.parametrize('name', sorted(IMRESIZE))
def test_post_ref_imresize_reproduces_fixture(R, name):
    c = IMRESIZE[name]
    kw = json.loads(str(c['kwargs']))
    out = R.imresize(c['x'], **kw)
    if c['out'].dtype == np.uint8:
        np.testing.assert_array_equal(out, c['out'])
    else:
        assert out.shape == c['out'].shape
        assert np.max(np.abs(out - c['out'])) <= 1e-6


@pytest.mark.parametrize('path', PYR, ids=[os.path.basename(p)[9:-4] for p in PYR])
def test_post_ref_pyramid_reproduces_fixture(R, path):
    z = np.load(path)
    kw = json.loads(str(z['kwargs']))
    ref = z['reference_u8'].transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    out = R.pyramid_upsampling(z['target'], ref, **kw)
    assert out.shape == z['out'].shape
    assert np.max(np.abs(out - z['out'])) <= 1e-6


def test_pyramid_fixture_semantics(R):
    z = np.load(os.path.join(GOLDEN_DIR, 'post_pyr_pad_150x100_l5.npz'))
    assert z['out'].shape == (3, 160, 128)                     # padded up to multiples of 2**5, and kept
    z = np.load(os.path.join(GOLDEN_DIR, 'post_pyr_s0_128x96_l4.npz'))
    np.testing.assert_allclose(z['out'], z['reference_u8'].transpose(2, 0, 1) / 255.0, atol=1e-6)   # no swap
    z = np.load(os.path.join(GOLDEN_DIR, 'post_pyr_l1_96x64.npz'))
    t = R.imresize(np.clip(z['target'], 0, 1).transpose(1, 2, 0), output_shape=(96, 64)).transpose(2, 0, 1)
    np.testing.assert_allclose(z['out'], t, atol=1e-6)         # one level: the resized, clamped target


@pytest.mark.parametrize('name', sorted(MKLC))
def test_post_ref_mkl_reproduces_fixture(R, name):
    c = MKLC[name]
    out, T = R.color_transfer(c['source'], c['target'])
    np.testing.assert_allclose(T, c['T'], rtol=1e-10, atol=1e-12)
    assert np.max(np.abs(out - c['out'])) <= 1e-6


def test_level_weights_and_errors(L):
    from histogan_amd.post import level_weights
    assert level_weights(5, 1, False) == [(1.0, 0.0)] + [(0.0, 1.0)] * 4
    w = level_weights(4, 1, True)
    assert w[0] == (1.0, 0.0) and w[1] == pytest.approx((2 / 3, 1 / 3)) and w[3] == pytest.approx((0.0, 1.0))
    with pytest.raises(IndexError):
        level_weights(5, 2, True)
    with pytest.raises(IndexError):
        level_weights(3, 4, False)
    with pytest.raises(ValueError):
        level_weights(0, 0, False)


def test_cabi_rejects_bad_arguments(L):
    lib, p = L.lib, ctypes.c_void_p(16)           # a non-null pointer that is never dereferenced: nothing launches
    EINVAL, EWS = -1, -4
    args = [p, 0, 1, 4, 1, 0, p, 0, 16, 4, 1, 3, 4, 4, 0, p, p, 8, 4, None]
    assert lib.hg_resize_axis(*args[:6], None, *args[7:]) == EINVAL
    for pos, bad in ((0, None), (15, None), (16, None), (11, 0), (12, 0), (13, -1), (14, 2), (17, 0), (18, 0),
                     (18, -3)):
        a = list(args)
        a[pos] = bad
        assert lib.hg_resize_axis(*a) == EINVAL, (pos, bad)
    assert lib.hg_pyr_down(None, p, 3, 8, 8, None) == EINVAL
    assert lib.hg_pyr_down(p, p, 3, 0, 8, None) == EINVAL
    assert lib.hg_pyr_down(p, p, 0, 8, 8, None) == EINVAL
    assert lib.hg_pyr_up_add(None, None, None, 0.0, None, None, 0.0, p, 3, 4, 4, None) == EINVAL
    assert lib.hg_pyr_up_add(p, None, None, 0.0, None, None, 0.0, p, 3, 0, 4, None) == EINVAL
    assert lib.hg_pyr_up_add(p, None, p, 1.0, None, None, 0.0, p, 3, 4, 4, None) == EINVAL    # weight without data
    assert lib.hg_pyr_up_add(p, None, None, 0.0, p, None, 0.5, p, 3, 4, 4, None) == EINVAL
    assert lib.hg_color_moments_workspace_bytes(1) == 0 and lib.hg_color_moments_workspace_bytes(10 ** 7) > 0
    assert lib.hg_color_moments(p, 1, 3, 1, p, p, 1 << 20, None) == EINVAL
    assert lib.hg_color_moments(p, 100, 0, 1, p, p, 1 << 20, None) == EINVAL
    assert lib.hg_color_moments(None, 100, 3, 1, p, p, 1 << 20, None) == EINVAL
    assert lib.hg_color_moments(p, 10 ** 7, 3, 1, p, p, 8, None) == EWS
    coef = (ctypes.c_float * 15)()
    assert lib.hg_color_affine(p, 0, 3, 1, coef, p, 0, None) == EINVAL
    assert lib.hg_color_affine(p, 10, 3, 1, None, p, 0, None) == EINVAL
    assert lib.hg_color_affine(None, 10, 3, 1, coef, p, 1, None) == EINVAL
    assert lib.hg_u8_hwc_to_f32(p, None, 3, 10, None) == EINVAL
    assert lib.hg_u8_hwc_to_f32(p, p, 3, 0, None) == EINVAL
    assert lib.hg_f32_to_u8_hwc(None, p, 3, 10, None) == EINVAL
    assert lib.hg_f32_to_u8_hwc(p, p, 0, 10, None) == EINVAL
