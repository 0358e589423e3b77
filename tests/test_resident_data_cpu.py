"""Device-resident image folder, the part that needs no device: the integer tables of Pillow's 8-bit bilinear resize
(histogan_amd.data.pil_bilinear_tables) with the numpy passes of tests/pilresize_ref.py equal `Image.resize(..., BILINEAR,
box=...)` byte for byte, the tables keep the invariants the kernel relies on, and the argument rules of ResidentFolderData
and of the C ABI of include/hg_data.h refuse what they should before anything is launched.

Before the feature every test here fails for want of the names it imports."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pilresize_ref as R
from histogan_amd.data import ResidentFolderData, pil_bilinear_tables, stage1_size


def _cases(n=240):
    """(img, size, box) -- seeded; sides 5..90, outputs 3..70; odd cases take integer boxes (some touching each border), even
    ones fractional boxes; every 7th keeps its width (an identity axis when its box covers it), every 11th reduces the
    height by more than 13x; plus fixed cases: identity on both axes, a pure up-scale, a reduction of 3.5x (ksize 9)."""
    rs = np.random.RandomState(0)
    out = []
    for k in range(n):
        h, w = (int(v) for v in rs.randint(5, 91, 2))
        oh, ow = (int(v) for v in rs.randint(3, 71, 2))
        if k % 7 == 0:
            ow = w if w <= 70 else ow
        if k % 11 == 0:
            h, oh = int(rs.randint(40, 91)), 3
        img = (rs.rand(h, w, 3) * 255).astype(np.uint8)
        if k % 2:
            l = int(rs.randint(0, w - 1)); r = int(rs.randint(l + 1, w + 1))
            t = int(rs.randint(0, h - 1)); b = int(rs.randint(t + 1, h + 1))
            if k % 5 == 0:
                l, t = 0, 0
            if k % 3 == 0:
                r, b = w, h
            if k % 14 == 7:
                l, r = 0, w                                    # the box covers a kept width: that pass is the identity
        else:
            l = rs.uniform(0, w - 1.5); r = rs.uniform(l + 1, w)
            t = rs.uniform(0, h - 1.5); b = rs.uniform(t + 1, h)
        out.append((img, (ow, oh), (l, t, r, b)))
    img = (rs.rand(28, 63, 3) * 255).astype(np.uint8)
    out.append((img, (63, 28), (0, 0, 63, 28)))                # identity
    out.append((img[:9, :9].copy(), (16, 16), (0, 0, 9, 9)))   # 9 -> 16 up-scale
    out.append((img, (18, 8), (0, 0, 63, 28)))                 # 3.5x: ksize 9
    return out


def test_tables_and_reference_passes_equal_pillow():
    from PIL import Image
    cases = _cases()
    assert len(cases) >= 200
    kinds = set()
    for img, size, box in cases:
        want = np.asarray(Image.fromarray(img).resize(size, Image.BILINEAR, box=box))
        got = R.resize(img, size, box, tables_fn=pil_bilinear_tables)
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), (img.shape, size, box)
        assert np.array_equal(R.resize(img, size, box), want), (img.shape, size, box)      # the plain-loop tables too
        for in_size, in0, in1, n_out in ((img.shape[1], box[0], box[2], size[0]), (img.shape[0], box[1], box[3], size[1])):
            scale = (in1 - in0) / n_out
            ksize = pil_bilinear_tables(in_size, in0, in1, n_out)[1].shape[1]
            kinds.add('identity' if (n_out == in_size and in0 == 0 and in1 == in_size) else 'up' if scale < 1 else
                      'k9' if scale > 3 and ksize == 9 else 'other')
    assert {'identity', 'up', 'k9'} <= kinds


def test_identity_tables_copy_the_axis():
    bounds, coeffs = pil_bilinear_tables(23, 0, 23, 23)
    assert coeffs.shape == (23, 3) and np.array_equal(bounds[:, 0], np.arange(23))
    assert np.array_equal(coeffs[:, 0], np.full(23, 1 << 22)) and not coeffs[:, 1:].any()


def test_table_invariants():
    rs = np.random.RandomState(3)
    for k in range(300):
        in_size, n_out = int(rs.randint(1, 400)), int(rs.randint(1, 300))
        if k % 2:
            in0 = int(rs.randint(0, in_size)); in1 = int(rs.randint(in0 + 1, in_size + 1))
        else:
            in0 = rs.uniform(0, in_size - 0.5); in1 = rs.uniform(in0 + 0.25, in_size)
        bounds, coeffs = pil_bilinear_tables(in_size, in0, in1, n_out)
        scale = float(np.float32(in1) - np.float32(in0)) / n_out          # Pillow takes the box as floats
        ksize = int(np.ceil(max(scale, 1.0))) * 2 + 1
        assert bounds.dtype == np.int32 and coeffs.dtype == np.int32
        assert bounds.shape == (n_out, 2) and coeffs.shape == (n_out, ksize)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 0).all() and (bounds[:, 1] <= ksize).all()
        assert (bounds[:, 0] + bounds[:, 1] <= in_size).all()
        assert (coeffs >= 0).all()                               # the triangle filter has no negative lobe
        assert (np.abs(coeffs.sum(axis=1, dtype=np.int64) - (1 << 22)) <= ksize).all()
        for o in range(n_out):
            assert not coeffs[o, bounds[o, 1]:].any()            # nothing past a row's taps
    a, b = pil_bilinear_tables(64, 0, 64, 16), pil_bilinear_tables(64, 0, 64, 16)
    assert a[0] is b[0] and not a[1].flags.writeable             # cached, and safe to share
    with pytest.raises(ValueError):
        pil_bilinear_tables(10, 4, 4, 5)


def test_stage1_size_is_the_resize_of_load_rgb():
    assert stage1_size(40, 30, 16) == (int(16 * 40 / 30), 16) and stage1_size(30, 40, 16) == (16, int(16 * 40 / 30))
    assert stage1_size(97, 130, 16) == (16, 21) and stage1_size(16, 50, 16) == (16, 50) and stage1_size(20, 20, 16) == (16, 16)


class _NoHist:
    def __call__(self, x):
        raise AssertionError('not reached')


def test_argument_rules(tmp_path):
    from PIL import Image
    Image.fromarray(np.zeros((20, 20, 3), np.uint8)).save(os.path.join(tmp_path, 'a.png'))
    cpu = torch.device('cpu')
    with pytest.raises(ValueError, match='premultiplied alpha') as e:
        ResidentFolderData(str(tmp_path), _NoHist(), 2, 16, cpu, transparent=True)
    assert 'FolderData' in str(e.value) and 'transparent' in str(e.value)
    with pytest.raises(FileNotFoundError):
        ResidentFolderData(str(tmp_path / 'nothing_here'), _NoHist(), 1, 16, cpu)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        ResidentFolderData(str(tmp_path), _NoHist(), 1, 16, cpu)


def test_trainer_keyword_is_an_extra_with_a_default():
    import inspect
    from histoGAN import Trainer
    from ReHistoGAN.rehistoGAN import recoloringTrainer
    for cls, names in ((Trainer, ['folder', 'resident']), (recoloringTrainer, ['folder', 'sampling', 'resident'])):
        sig = inspect.signature(cls.set_data_src)
        assert [p for p in sig.parameters if p != 'self'] == names and sig.parameters['resident'].default is False


def test_transparent_trainer_is_refused_when_the_source_is_set(tmp_path):
    """set_data_src(folder, resident=True) of a transparent trainer raises the source's ValueError (the methods are called on
    a stand-in that carries the attributes they read: no network is built for this)."""
    import types
    from PIL import Image
    from histoGAN import Trainer
    from ReHistoGAN.rehistoGAN import recoloringTrainer
    Image.fromarray(np.zeros((20, 20, 3), np.uint8)).save(os.path.join(tmp_path, 'a.png'))
    stub = types.SimpleNamespace(histBlock=_NoHist(), batch_size=2, image_size=16, device=torch.device('cpu'), transparent=True,
                                 dataset_aug_prob=0.0, hist_alpha_weight=False)
    for cls in (Trainer, recoloringTrainer):
        with pytest.raises(ValueError, match='premultiplied alpha'):
            cls.set_data_src(stub, str(tmp_path), resident=True)
        cls.set_data_src(stub, str(tmp_path))                   # the default still serves RGBA
        assert stub.loader.rgba and type(stub.loader).__name__ == 'FolderData'


@pytest.fixture(scope='module')
def L():
    from histogan_amd import build
    build.build()
    import histogan_amd._lib as L
    return L


def test_cabi_refuses_before_any_launch(L):
    lib = L.lib
    assert lib.hg_version() >= 115
    assert lib.hg_data_item_bytes() == ctypes.sizeof(L.HgDataItem) == 56
    from histogan_amd.data import ITEM_DTYPE
    assert ITEM_DTYPE.itemsize == 56
    assert [ITEM_DTYPE.fields[n][1] for n in ITEM_DTYPE.names] == [getattr(L.HgDataItem, n).offset for n in ITEM_DTYPE.names]
    kmax = lib.hg_data_max_ksize()
    assert kmax >= 9
    p = ctypes.c_void_p(4096)                  # never dereferenced: every call below returns before a launch
    EINVAL = -1
    ok = dict(items=p, n=2, axis=1, max_bytes=768, bounds=p, coeffs=p, n_tab=32, ksize=3)

    def resample(**kw):
        a = dict(ok, **kw)
        return lib.hg_data_resample_axis(a['items'], a['n'], a['axis'], a['max_bytes'], a['bounds'], a['coeffs'], a['n_tab'],
                                         a['ksize'], None)
    for bad in (dict(items=None), dict(bounds=None), dict(coeffs=None), dict(n=0), dict(n=-3), dict(n=65536), dict(axis=2),
                dict(ksize=0), dict(ksize=kmax + 1), dict(n_tab=0), dict(max_bytes=0), dict(max_bytes=1 << 31)):
        assert resample(**bad) == EINVAL, bad
    assert lib.hg_data_finish(None, 2, 16, p, None) == EINVAL and lib.hg_data_finish(p, 2, 16, None, None) == EINVAL
    assert lib.hg_data_finish(p, 0, 16, p, None) == EINVAL and lib.hg_data_finish(p, 65536, 16, p, None) == EINVAL
    assert lib.hg_data_finish(p, 2, 0, p, None) == EINVAL and lib.hg_data_finish(p, 2, 16385, p, None) == EINVAL
