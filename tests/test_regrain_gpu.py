"""Regrain on the GPU (hg_regrain_*, include/hg_regrain.h; post.regrain; recoloringTrainer.evaluate(post_recoloring=
'idt_regrain')) against the numpy restatement tests/regrain_ref.py, stage by stage with the inputs handed in.

Bars:
  begin, finish   exact: E is one correctly rounded fp32 subtraction, J one addition and a clip; quantize truncates v * 255
  coef            every plane within 16 * 2^-24 RELATIVE of the fp64 value: the chain to any plane is fewer than 16 correctly
                  rounded differences, products, positive sums, square roots and quotients
  sweep           16 n 2^-24 max|E| against the fp64 sweeps on the GPU's own coefficient planes: the update is a convex
                  combination, so the rounding of one sweep (at most 16 operations) is not amplified by the next
  fused           every setting of `fused` gives the bits of fused = 1
  whole chain     8 x the largest difference between regrain_ref in float32 and in float64 on the same inputs (8 for the fused
                  multiply-adds of the kernel, which the numpy float32 run does not have), plus 1e-5 -- the bar of the resize in
                  tests/test_post_gpu.py -- per level below the first
Shapes come from hg_regrain_tile_h / _tile_w / _max_fused.  The measured errors are in DESIGN.md section 6j."""
import numpy as np
import pytest
import torch

import regrain_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
EPS = 2.0 ** -24


@pytest.fixture(scope='module')
def P():
    from histogan_amd import build
    build.build()
    from histogan_amd import post
    return post


@pytest.fixture(scope='module')
def K(P):
    return dict(th=P.lib.hg_regrain_tile_h(), tw=P.lib.hg_regrain_tile_w(), kmax=P.lib.hg_regrain_max_fused())


def shapes(K):
    th, tw = K['th'], K['tw']
    return [(2, 2), (2, 3), (3, 5), (th, tw), (th + 1, tw + 1), (2 * th + 3, tw - 1), (th + 1, 2 * tw + 4), (7, tw + 6)]


def image(h, w, seed):
    """(h, w, 3) fp32 in [0, 1]: flat bands (d = 0), ramps whose slope passes through 5 / 256 (psi straddles 1), texture."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    slope = (5.0 / 256.0) * (0.25 + 1.5 * yy / max(h - 1, 1)) / np.sqrt(3.0)
    img = np.stack([(0.1 + slope * xx) % 1.0] * 3, -1)
    img[:, : w // 3] = np.array([0.25, 0.5, 0.75])                     # flat: every gradient is exactly 0
    tex = rs.uniform(0, 1, (h, w, 3))
    img[h // 2:, w // 2:] = tex[h // 2:, w // 2:]
    return np.clip(img, 0, 1).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_begin(P, o, t):
    """hg_regrain_begin on two (H, W, 3) device views: the planes (I, E)."""
    src, _, ps0, cs0 = P._pixels(o, 'original', 'regrain')
    tgt, _, ps1, cs1 = P._pixels(t, 'transferred', 'regrain')
    H, W = o.shape[:2]
    I, E = torch.empty(3, H, W, device=DEV), torch.empty(3, H, W, device=DEV)
    P.check(P.lib.hg_regrain_begin(src.data_ptr(), ps0, cs0, tgt.data_ptr(), ps1, cs1, H, W, I.data_ptr(), E.data_ptr(),
                                   P.raw_stream(DEV)), 'hg_regrain_begin')
    return I, E


def gpu_coef(P, I, level, smoothness=1.0):
    _, H, W = I.shape
    C, scratch = torch.empty(4, H, W, device=DEV), torch.empty(H, W, device=DEV)
    P.check(P.lib.hg_regrain_coef(I.data_ptr(), H, W, level, smoothness, C.data_ptr(), scratch.data_ptr(), P.raw_stream(DEV)),
            'hg_regrain_coef')
    return C


def gpu_sweep(P, D0, E, C, n, fused):
    a, b = D0.clone(), torch.full_like(D0, float('nan'))
    return P.regrain_sweep(a, b, E, C, n, fused).clone()


def gpu_finish(P, I, D, quantize):
    _, H, W = I.shape
    out = torch.empty(H, W, 3, dtype=torch.uint8 if quantize else torch.float32, device=DEV)
    P.check(P.lib.hg_regrain_finish(I.data_ptr(), D.data_ptr(), H, W, out.data_ptr(), int(quantize), P.raw_stream(DEV)),
            'hg_regrain_finish')
    return out


def level_inputs(P, h, w, seed, level=0):
    """A level's planes on the device: (D0, E, C) with E and D0 random in [-0.3, 0.3] and C the GPU's coefficients of image()."""
    rs = np.random.RandomState(1000 + seed)
    I = dev(image(h, w, seed).transpose(2, 0, 1))
    E = dev(rs.uniform(-0.3, 0.3, (3, h, w)).astype(np.float32))
    D0 = dev(rs.uniform(-0.3, 0.3, (3, h, w)).astype(np.float32))
    return D0, E, gpu_coef(P, I, level)


# ---- begin and finish ------------------------------------------------------------------------------------------------------
def test_begin_and_finish_are_exact_for_every_layout(P, K):
    for n, (h, w) in enumerate(shapes(K)):
        rs = np.random.RandomState(n)
        o, t = image(h, w, n), rs.uniform(-0.2, 1.2, (h, w, 3)).astype(np.float32)
        chw = dev(o.transpose(2, 0, 1))                                  # a CHW image, viewed as (H, W, 3)
        wide = dev(np.concatenate([o, o[..., :2]], -1))                  # five channels, the first three taken
        wide[..., 3:] = 7.0
        padded = dev(np.concatenate([o, o[:, :2]], 1))                   # rows two pixels longer than the image
        views = [dev(o), chw.permute(1, 2, 0), wide[..., :3], padded[:, :w]]
        for v in views:
            before = v.clone()
            I, E = gpu_begin(P, v, dev(t))
            assert torch.equal(v, before)
            assert np.array_equal(I.cpu().numpy(), o.transpose(2, 0, 1))
            assert np.array_equal(E.cpu().numpy(), (t - o).transpose(2, 0, 1))          # numpy's fp32 subtraction rounds once
        D = dev(rs.uniform(-0.6, 0.6, (3, h, w)).astype(np.float32))
        want = np.clip((I.cpu().numpy() + D.cpu().numpy()), np.float32(0), np.float32(1)).transpose(1, 2, 0)
        got = gpu_finish(P, I, D, False)
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want)
        assert h * w < 64 or (want.min() == 0 and want.max() == 1)      # both clips are exercised
        q = gpu_finish(P, I, D, True)
        assert q.dtype == torch.uint8 and np.array_equal(q.cpu().numpy(), (want * np.float32(255)).astype(np.uint8))


# ---- coefficients ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('level', [0, 3, 5])
def test_coefficient_planes_within_16_ulp_relative_of_fp64(P, K, level):
    for n, (h, w) in enumerate(shapes(K)):
        for smoothness in (1.0, 0.3):
            img = image(h, w, n)
            got = gpu_coef(P, dev(img.transpose(2, 0, 1)), level, smoothness).cpu().numpy().astype(np.float64)
            want = R.coef(img.transpose(2, 0, 1).astype(np.float64), level, float(np.float32(smoothness)))
            err = np.abs(got - want)
            rel = float(np.max(err / np.maximum(np.abs(want), 1e-300)))
            print(f'coef {h}x{w} level {level} smoothness {smoothness}: max relative error {rel / EPS:.2f} x 2^-24')
            assert np.all(err <= 16 * EPS * np.abs(want)), (h, w, rel / EPS)
            if h * w >= 64:
                d = R.gradient_magnitude(img.transpose(2, 0, 1).astype(np.float64))
                assert (d == 0).any() and (256 * d / 5 < 1).any() and (256 * d / 5 > 1).any() and (want[0] == 0).any()
            assert np.all(got[1][:, -1] == 0) and np.all(got[2][-1, :] == 0) and np.all(got[3] > 0)


# ---- the sweep ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 4, 5, 64])
def test_sweeps_against_fp64_on_the_gpus_own_coefficients(P, K, n):
    for seed, (h, w) in enumerate(shapes(K)):
        D0, E, C = level_inputs(P, h, w, seed, level=seed % 3)
        want = R.sweep(D0.cpu().numpy().astype(np.float64), E.cpu().numpy().astype(np.float64),
                       C.cpu().numpy().astype(np.float64), n)
        bar = 16 * n * EPS * float(E.abs().max())
        for fused in (1, 0, min(3, K['kmax'])):
            got = gpu_sweep(P, D0, E, C, n, fused).cpu().numpy()
            err = float(np.max(np.abs(got - want)))
            print(f'sweep {h}x{w} n {n} fused {fused}: error {err:.3e}, bar {bar:.3e}')
            assert err <= bar


def test_every_fused_setting_gives_the_bits_of_one_sweep_per_launch(P, K):
    kmax = K['kmax']
    for seed, (h, w) in enumerate(shapes(K)):
        D0, E, C = level_inputs(P, h, w, seed)
        keep = (D0.clone(), E.clone(), C.clone())
        for n in (1, 5, 8):                  # below k; a multiple of k = 5 and not of 2, 3, 4; a multiple of 2, 4, 8 and not of 3, 5, 6, 7
            base = gpu_sweep(P, D0, E, C, n, 1)
            assert torch.isfinite(base).all()
            for fused in [0] + list(range(2, kmax + 1)):
                got = gpu_sweep(P, D0, E, C, n, fused)
                assert torch.equal(got, base), (h, w, n, fused, float((got - base).abs().max()))
        assert torch.equal(D0, keep[0]) and torch.equal(E, keep[1]) and torch.equal(C, keep[2])
    # the result lands in the buffer the launch count says
    D0, E, C = level_inputs(P, 9, 12, 0)
    for n, fused in ((4, 1), (5, 1), (5, 2), (8, 3), (7, 8)):
        a, b = D0.clone(), torch.full_like(D0, float('nan'))
        r = P.regrain_sweep(a, b, E, C, n, fused)
        assert (r is b) == (P.lib.hg_regrain_sweep_launches(n, fused) % 2 == 1) and torch.isfinite(r).all()


def test_resize_into_the_workspace_equals_imresize(P):
    x = dev(np.random.RandomState(3).uniform(-1, 1, (3, 37, 50)).astype(np.float32))
    for hw in ((19, 25), (74, 100), (19, 100)):
        out = torch.empty(3, *hw, device=DEV)
        assert torch.equal(P._resize_planes_into(x, out), P.imresize(x, output_shape=hw, method='bilinear'))


# ---- the whole chain ---------------------------------------------------------------------------------------------------------
CHAIN = [((9, 7), dict(min_side=2)), ((9, 7), dict(min_side=1)), ((37, 50), dict(min_side=2)), ((96, 128), dict())]


@pytest.mark.parametrize('hw,kw', CHAIN, ids=lambda v: str(v).replace(' ', ''))
def test_regrain_against_the_reference(P, hw, kw):
    I, T = (v.astype(np.float32) for v in R.synthetic_pair(*hw))
    levels = len(R.levels(*hw, R.ITERATIONS, kw.get('min_side', R.MIN_SIDE)))
    if hw == (9, 7):
        assert levels == (3 if kw['min_side'] == 1 else 2)             # 9x7 -> 5x4 -> 3x2, and 2 does not exceed min_side = 2
    ref64 = R.regrain(I, T, dtype=np.float64, **kw)
    ref32 = R.regrain(I, T, dtype=np.float32, **kw)
    eps32 = float(np.max(np.abs(ref32 - ref64)))
    bar = 8 * eps32 + 1e-5 * (levels - 1)
    o, t = dev(I), dev(T)
    keep = (o.clone(), t.clone())
    got = P.regrain(o, t, **kw)
    assert got.dtype == torch.float32 and got.shape == (*hw, 3)
    err = float(np.max(np.abs(got.cpu().numpy() - ref64)))
    print(f'regrain {hw} {kw}: {levels} levels, fp32-fp64 reference {eps32:.3e}, bar {bar:.3e}, GPU error {err:.3e}')
    assert err <= bar
    assert torch.equal(o, keep[0]) and torch.equal(t, keep[1])
    for fused in (1, 2, P.REGRAIN_MAX_FUSED):
        assert torch.equal(P.regrain(o, t, fused=fused, **kw), got)
    assert torch.equal(P.regrain(o, t, **kw), got)                       # a second call: the same bits
    q = P.regrain(o, t, quantize=True, **kw)
    assert q.dtype == torch.uint8 and torch.equal(q, (got * 255).to(torch.uint8))
    chw = dev(I.transpose(2, 0, 1))
    assert torch.equal(P.regrain(chw.permute(1, 2, 0), t, **kw), got)    # a CHW original


def test_regrain_of_a_picture_with_itself_is_the_picture(P, K):
    for n, (h, w) in enumerate(shapes(K) + [(96, 128)]):
        x = dev(image(h, w, n))
        assert torch.equal(P.regrain(x, x.clone(), min_side=2), x)
        assert torch.equal(P.regrain(x, x.clone(), quantize=True), (x * 255).to(torch.uint8))


def test_regrain_effect_on_the_gpu(P):
    """The CPU effect test's pair: the gradient mismatch to the original falls to a fifth or less, and the result stays closer
    to the transferred picture than the original is."""
    I, T = R.synthetic_pair()
    J = P.regrain(dev(I.astype(np.float32)), dev(T.astype(np.float32))).cpu().numpy()
    assert R.gradient_rms(J, I) <= 0.2 * R.gradient_rms(T, I)
    assert np.abs(J - T).mean() < np.abs(T - I).mean()


# ---- recoloringTrainer.evaluate ------------------------------------------------------------------------------------------------
def test_evaluate_post_recoloring_idt_regrain(P, tmp_path, monkeypatch):
    torch.manual_seed(0)
    from ReHistoGAN.rehistoGAN import recoloringTrainer
    tr = recoloringTrainer('regrain', str(tmp_path / 'results'), str(tmp_path / 'models'), image_size=64, network_capacity=4,
                           batch_size=1, hist_bin=16, hist_insz=32)
    tr.init_GAN()
    rs = np.random.RandomState(4)
    photo = np.clip(0.5 + 0.25 * np.sin(np.mgrid[0:40, 0:52][0][..., None] / 6.0 + np.arange(3)) + rs.normal(0, 0.05, (40, 52, 3)),
                    0, 1)
    photo = np.round(photo * 255) / 255
    img = torch.rand(1, 3, 64, 64, device=DEV)
    h = torch.rand(1, 3, 16, 16, device=DEV)
    h = h / h.sum(dim=(1, 2, 3), keepdim=True)
    writes = []
    real = P.save_rgb
    monkeypatch.setattr(P, 'save_rgb', lambda a, p: (writes.append(a.clone()), real(a, p)))
    src = torch.from_numpy(np.ascontiguousarray(photo, dtype=np.float32)).to(DEV)
    with torch.no_grad():
        g = tr.evaluate('out_regrain', image_batch=img, hist_batch=h, original_image=photo, save_input=False,
                        post_recoloring='idt_regrain')
    assert len(writes) == 1 and writes[0].dtype == torch.uint8 and writes[0].shape == (40, 52, 3)
    moved = P.color_transfer_idt(src, g[0].permute(1, 2, 0))[0]
    assert torch.equal(writes[0], P.regrain(src, moved, quantize=True))
    old = P.color_transfer_idt(src, g[0].permute(1, 2, 0), quantize=True)[0]
    assert not torch.equal(writes.pop(), old)
    with torch.no_grad():
        g2 = tr.evaluate('out_idt', image_batch=img, hist_batch=h, original_image=photo, save_input=False, post_recoloring='idt')
    assert len(writes) == 1 and torch.equal(writes[0], P.color_transfer_idt(src, g2[0].permute(1, 2, 0), quantize=True)[0])
