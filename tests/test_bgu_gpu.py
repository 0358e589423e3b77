"""Bilateral guided upsampling on the GPU (hg_bgu_normal, hg_bgu_slice, histogan_amd/post.py's bgu_* and
recoloringTrainer.evaluate(resizing_method='BGU_native')) against the fp64 oracle tests/bgu_oracle.py, which solves the
stacked least-squares system with QR and shares no structure with the code under test.

Bars.
* A^T W A and A^T W out, fp64 against fp64, as a fraction of the largest entry.  A plain numpy `A.T @ (w * A)` of the
  oracle's rows differs from the same product in long double by at most 8.52e-16 of the largest entry over the six
  cases used here (three shapes, with and without weights; 1.9e-16 at the best), and `A.T @ (w * out)` by at most
  7.3e-16 (bgu_oracle.PLAIN_ATA_ERR / PLAIN_ATB_ERR; tests/test_bgu_cpu.py recomputes both); times 10 for the
  summation order gives NORMAL_BAR = 8.52e-15 and RHS_BAR = 7.3e-15.
* Every float image: FLOAT_BAR = 0.01 / 255 (3.9e-5), so that a byte can only differ from the oracle's where the
  oracle's unrounded 255 v lies within DELTA = 0.01 of a rounding boundary.  Bytes must be equal everywhere else, and at
  most 4 % of the values may be excused that way (2 % of evenly spread fractions fall in the band).
Every test prints the figure it then asserts."""
import numpy as np
import pytest
import torch

import bgu_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
NORMAL_BAR = 10 * O.PLAIN_ATA_ERR
RHS_BAR = 10 * O.PLAIN_ATB_ERR
DELTA = 0.01
FLOAT_BAR = DELTA / 255
EXCUSED_CAP = 0.04
SHAPES = O.LOWRES_SHAPES


@pytest.fixture(scope='module')
def P():
    from histogan_amd import build
    build.build()
    from histogan_amd import post
    return post


pair = O.lowres_case


def chw(a):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(DEV)


def check_bytes(got, v, what):
    """got == round(255 clip(v)) except where the oracle's value is within DELTA of a rounding boundary."""
    want, raw = O.quantize(v)
    mask = O.excused(raw, DELTA)
    bad = (got != want) & ~mask
    print(f'{what}: excused {float(mask.mean()):.4f}, differing bytes {int((got != want).sum())}, not excused {int(bad.sum())}')
    assert got.shape == want.shape and got.dtype == np.uint8
    assert float(mask.mean()) <= EXCUSED_CAP
    assert not bad.any()
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('h,w', SHAPES)
def test_normal_equations_vs_oracle(P, h, w, weighted):
    in_ds, out_ds, wt = pair(h, w)
    grid = O.grid_size(h, w)
    A = O.data_rows(in_ds.astype(np.float64), grid)
    wv = wt.astype(np.float64).reshape(-1) if weighted else np.ones(h * w)
    N = A.T @ (wv[:, None] * A)
    b = A.T @ (wv[:, None] * out_ds.reshape(-1, 3).astype(np.float64))
    want_d, want_o, outside = O.slab_blocks(N, grid)
    assert outside == 0.0
    S, m = want_d.shape[:2]
    want_r = b[O.slab_permutation(grid)].T.reshape(3, S, m)
    wd = torch.from_numpy(wt).to(DEV) if weighted else None
    diag, off, rhs = P.bgu_normal(chw(in_ds), chw(out_ds), wd)
    again = P.bgu_normal(chw(in_ds), chw(out_ds), wd)
    assert diag.dtype == torch.float64 and tuple(diag.shape) == (S, m, m) and tuple(off.shape) == (S - 1, m, m)
    scale, rscale = np.max(np.abs(N)), np.max(np.abs(b))
    ed = np.max(np.abs(diag.cpu().numpy() - want_d)) / scale
    eo = np.max(np.abs(off.cpu().numpy() - want_o)) / scale
    er = np.max(np.abs(rhs.cpu().numpy() - want_r)) / rscale
    print(f'normal {h}x{w} weighted={weighted}: diag {ed:.2e} off {eo:.2e} rhs {er:.2e} of the largest entry')
    assert max(ed, eo) <= NORMAL_BAR and er <= RHS_BAR
    for a, c in zip((diag, off, rhs), again):
        assert torch.equal(a, c)                                              # bit-identical repeats


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('h,w', SHAPES)
def test_fit_vs_oracle(P, h, w, weighted):
    """gamma in cells no pixel reaches is held by the 4e-7 regulariser alone, so the fits are compared through the
    low-resolution image they produce."""
    in_ds, out_ds, wt = pair(h, w)
    i64, o64 = in_ds.astype(np.float64), out_ds.astype(np.float64)
    want = O.fit(i64, o64, wt.astype(np.float64) if weighted else None)
    gamma = P.bgu_fit(chw(in_ds), chw(out_ds), torch.from_numpy(wt).to(DEV) if weighted else None)
    assert gamma.dtype == torch.float32 and tuple(gamma.shape) == want.shape
    err = np.max(np.abs(O.slice_(gamma.cpu().numpy().astype(np.float64), i64) - O.slice_(want, i64)))
    print(f'fit {h}x{w} weighted={weighted}: sliced low-resolution max abs {err:.2e}')
    assert err <= FLOAT_BAR


@pytest.mark.parametrize('H,W,pad', [(131, 97, 0), (131, 97, 2), (9, 601, 0), (9, 601, 1)])
def test_slice_random_gamma(P, H, W, pad):
    """The slice alone: a random grid, odd photo sizes, rows that start at every byte alignment (pad > 0: a
    non-contiguous row stride), one and several tiles per row."""
    rng = np.random.default_rng(H + pad)
    gamma = (rng.normal(0, 0.4, (4, 5, 8, 3, 4))).astype(np.float32)
    photo = O.synthetic_photo(3, H, W)
    buf = torch.zeros((H, W + pad, 3), dtype=torch.uint8, device=DEV)
    view = buf[:, :W]
    view.copy_(torch.from_numpy(photo).to(DEV))
    assert view.is_contiguous() == (pad == 0)
    want = O.slice_(gamma.astype(np.float64), photo.astype(np.float64) / 255)
    g = torch.from_numpy(gamma).to(DEV)
    out = P.bgu_slice(g, view, quantize=False)
    assert out.dtype == torch.float32 and tuple(out.shape) == (3, H, W)
    err = np.max(np.abs(out.cpu().numpy().transpose(1, 2, 0) - want))
    print(f'slice {H}x{W} pad {pad}: fp32 max abs {err:.2e} (values up to {np.max(np.abs(want)):.2f})')
    assert err <= FLOAT_BAR
    u8 = P.bgu_slice(g, view, quantize=True)
    check_bytes(u8.cpu().numpy(), want, f'slice {H}x{W} pad {pad}')
    assert torch.equal(u8, P.bgu_slice(g, view, quantize=True))
    assert np.array_equal(view.cpu().numpy(), photo)


@pytest.mark.parametrize('max_side', [300, 40])
def test_upsampling_end_to_end(P, max_side):
    photo = O.synthetic_photo(11, 131, 97)
    target = O.synthetic_target(photo, 64, 48)
    want, _ = O.upsample(target, photo, max_side=max_side)
    pd, td = torch.from_numpy(photo).to(DEV), torch.from_numpy(target).to(DEV)
    out = P.bgu_upsampling(td.unsqueeze(0), pd, max_side=max_side)
    assert out.dtype == torch.float32 and tuple(out.shape) == (1, 3, 131, 97)           # the photo's size, no padding
    err = np.max(np.abs(out[0].cpu().numpy().transpose(1, 2, 0) - want))
    print(f'end to end max_side {max_side}: fp32 max abs {err:.2e} (bar {FLOAT_BAR:.2e})')
    assert err <= FLOAT_BAR
    u8 = P.bgu_upsampling(td, pd, max_side=max_side, quantize=True)
    check_bytes(u8.cpu().numpy(), want, f'end to end max_side {max_side}')
    assert np.array_equal(pd.cpu().numpy(), photo) and np.array_equal(td.cpu().numpy(), target)


def test_evaluate_bgu_native(P, tmp_path, monkeypatch):
    from PIL import Image
    torch.manual_seed(0)
    from ReHistoGAN.rehistoGAN import recoloringTrainer
    tr = recoloringTrainer('bgu', str(tmp_path / 'results'), str(tmp_path / 'models'), image_size=64,
                           network_capacity=4, batch_size=1, hist_bin=16, hist_insz=32)
    tr.init_GAN()
    photo = O.synthetic_photo(7, 200, 300)
    name = str(tmp_path / 'photo.png')
    Image.fromarray(photo).save(name)
    img = torch.rand(1, 3, 64, 64, device=DEV)
    h = torch.rand(1, 3, 16, 16, device=DEV)
    h = h / h.sum(dim=(1, 2, 3), keepdim=True)
    writes = []
    real = P.save_rgb
    monkeypatch.setattr(P, 'save_rgb', lambda a, p: (writes.append((a.cpu().numpy().copy(), p)), real(a, p)))
    with torch.no_grad():
        g = tr.evaluate('out', image_batch=img, hist_batch=h, resizing='upscaling', resizing_method='BGU_native',
                        input_image_name=name, save_input=False)
    out_name = str(tmp_path / 'results' / 'bgu' / 'out-generated.jpg')
    assert [p for _, p in writes] == [out_name]                                        # one write
    assert writes[0][0].shape == (200, 300, 3) and writes[0][0].dtype == np.uint8
    want = P.bgu_upsampling(g, torch.from_numpy(photo).to(DEV), quantize=True)
    assert np.array_equal(writes[0][0], want.cpu().numpy())
    with Image.open(out_name) as im:
        assert im.size == (300, 200)
