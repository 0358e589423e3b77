"""Differentiable 3D LUTs on the GPU (hg_lut_apply_bwd, hg_lut_adam_step, include/hg_lut.h version 118; post.lut_apply(
differentiable=True), lut_apply_backward, lut_adam_step, lut_refine; evaluate(post_recoloring='lut_refine')) against the numpy
restatement tests/lut_grad_ref.py.

glut     the integer sums in the workspace equal the restatement exactly (every quantity is an integer), and so do the bits of
         glut; against the fp64 reference the bar per node is count_j u + 2^-24 |ref_j|: twice the derived rounding bound of the
         contributions plus the one rounding to fp32.  The same bits for every source form, `blocks` value and run.
gx       4 eps32 against fp64 on the pixels where fp32 and fp64 agree about cell, ordering and masks (eps32: the reference in
         fp32 against fp64 arithmetic on those pixels); the rest are finite, and clamped or non-finite inputs give exactly 0.
adam     4 eps32 against fp64, one step and three chained.
refine   the per-step losses against the fp64 reference loop: 10 x the distance between the reference loop in fp32 and in fp64
         arithmetic at that step (DESIGN.md section 6k records the figures).
Every test prints what it measured.  On an MI355X: the integer sums and the bits of glut equal the restatement in every case, glut
errs by at most 0.997 of its bar; gx by 0.64 .. 1.2 eps32; the Adam step by exactly eps32 (it reproduces the fp32 restatement);
the refine's ratio |GPU - fp64| / |fp32 - fp64| is 9.68 at step 0 (both distances below 1e-7), 0.99 .. 1.03 at steps 1 .. 5 and
1.22 at step 50, and the weighted run equals the cropped one bit for bit."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import lut_grad_ref as G
import lut_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
INTERPOLATIONS = ('tetrahedral', 'trilinear')


@pytest.fixture(scope='module')
def P():
    from histogan_amd import build
    build.build()
    from histogan_amd import post
    return post


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def run(P, x, lut, g, interpolation, **kw):
    """(gx, glut, bits of gmax, integer sums) of one hg_lut_apply_bwd call on numpy inputs; x is (H, W, 3)."""
    ws = []
    gx, glut = P.lut_apply_backward(x if torch.is_tensor(x) else dev(x), dev(lut), dev(np.asarray(g, dtype=np.float32).reshape(x.shape)),
                                    interpolation, workspace_out=ws, **kw)
    n = lut.shape[0]
    raw = None if ws[0] is None else ws[0].cpu().numpy()
    gmax = None if raw is None else int(raw[:4].view(np.uint32)[0])
    sums = None if raw is None else raw[16:16 + n ** 3 * 24].view(np.int64).reshape(n, n, n, 3)
    return gx, glut, gmax, sums


@lru_cache(maxsize=None)
def standard(n):
    x = R.apply_image(n, seed=n)
    return x, R.random_lut(n, n), np.random.RandomState(100 + n).randn(x.shape[0] * x.shape[1], 3).astype(np.float32)


@lru_cache(maxsize=None)
def standard_ref(n, interpolation):
    x, lut, g = standard(n)
    return G.int_scatter(x, lut, g, interpolation), G.backward(x, lut, g, interpolation)


# ---- glut ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interpolation', INTERPOLATIONS)
@pytest.mark.parametrize('n', [2, 3, 17, 18, 33])
def test_glut_on_the_standard_inputs(P, n, interpolation):
    from histogan_amd._lib import lib
    assert lib.hg_lut_grad_lds_n() == 17                                  # 17 and 18 are its two sides
    x, lut, g = standard(n)
    val = G.pieces(x.reshape(-1, 3), lut, interpolation)[0]
    assert np.minimum(np.abs(val), np.abs(val - 1)).min() >= 1e-5         # fp32 and fp64 agree on every output mask
    (gmax, sums, counts, gl32, u), (_, ref) = standard_ref(n, interpolation)
    _, glut, got_gmax, got_sums = run(P, x, lut, g, interpolation)
    assert got_gmax == gmax
    assert np.array_equal(got_sums, sums)
    assert np.array_equal(bits(glut), gl32.view(np.uint32))
    err = np.abs(glut.cpu().numpy().astype(np.float64) - ref)
    bar = counts * u + 2.0 ** -24 * np.abs(ref)
    print(f'N = {n} {interpolation}: glut max err {err.max():.3e}, max |ref| {np.abs(ref).max():.2f}, u {u:.2e}, '
          f'largest err / bar {np.max(err / np.maximum(bar, 1e-300)):.3f}')
    assert np.all(err <= bar)


@pytest.mark.parametrize('interpolation', INTERPOLATIONS)
@pytest.mark.parametrize('n', [17, 33])
def test_glut_has_the_same_bits_for_every_source_form_block_count_and_run(P, n, interpolation):
    x, lut, g = standard(n)
    H, W = x.shape[:2]
    gx0, glut0, _, _ = run(P, x, lut, g, interpolation)
    chw = dev(x).permute(2, 0, 1).contiguous().permute(1, 2, 0)
    big = torch.full((H + 5, W + 7, 3), float('nan'), device=DEV)
    big[2:2 + H, 3:3 + W] = dev(x)
    forms = {'CHW view': chw, 'strided crop': big[2:2 + H, 3:3 + W], 'second run': dev(x)}
    for name, src in forms.items():
        assert src.shape == (H, W, 3)
        gx, glut, _, _ = run(P, src, lut, g, interpolation)
        assert torch.equal(gx, gx0) and np.array_equal(bits(glut), bits(glut0)), name
    for blocks in (1, 7, 512):
        gx, glut, _, _ = run(P, x, lut, g, interpolation, blocks=blocks)
        assert np.array_equal(bits(gx), bits(gx0)) and np.array_equal(bits(glut), bits(glut0)), blocks
    only_lut = run(P, x, lut, g, interpolation, want_image=False)
    only_x = run(P, x, lut, g, interpolation, want_lut=False)
    assert only_lut[0] is None and np.array_equal(bits(only_lut[1]), bits(glut0))
    assert only_x[1] is None and only_x[3] is None and np.array_equal(bits(only_x[0]), bits(gx0))


@lru_cache(maxsize=None)
def mild(n, npix, seed):
    """No output is clipped (entries in [0.1, 0.9]): the masks cannot depend on the arithmetic."""
    rs = np.random.RandomState(seed)
    return rs.rand(1, npix, 3).astype(np.float32), (0.1 + 0.8 * rs.rand(n, n, n, 3)).astype(np.float32), rs.randn(npix, 3).astype(np.float32)


@pytest.mark.parametrize('n,interpolation', [(17, 'tetrahedral'), (17, 'trilinear'), (33, 'tetrahedral'), (33, 'trilinear')])
def test_glut_pixel_counts_and_gradient_ranges(P, n, interpolation):
    for npix in (1, 3, 4, 5, 4095, 4096, 4097, 12286):
        x, lut, g = mild(n, npix, npix)
        gmax, sums, _, gl32, _ = G.int_scatter(x, lut, g, interpolation)
        gx, glut, got_gmax, got_sums = run(P, x, lut, g, interpolation)
        assert got_gmax == gmax and np.array_equal(got_sums, sums) and np.array_equal(bits(glut), gl32.view(np.uint32)), npix
        assert torch.isfinite(gx).all()
    x, lut, g = mild(n, 4097, 7)
    # one constant image: every contribution goes to one cell
    flat = np.broadcast_to(np.array([0.3, 0.6, 0.2], dtype=np.float32), x.shape).copy()
    ref = G.int_scatter(flat, lut, g, interpolation)
    _, glut, _, got_sums = run(P, flat, lut, g, interpolation)
    assert np.array_equal(got_sums, ref[1]) and np.count_nonzero(ref[1].any(axis=3)) in (4, 8)
    assert np.array_equal(bits(glut), ref[3].view(np.uint32))
    # g all zero: no unit, glut = 0
    _, glut, got_gmax, got_sums = run(P, x, lut, np.zeros_like(g), interpolation)
    assert got_gmax == 0 and not got_sums.any() and not bits(glut).any()
    # non-finite entries count as 0 and do not set the unit; nothing finite at all gives 0
    bad = g.copy()
    bad[::7, 0], bad[3::11, 1], bad[5::13, 2] = np.nan, np.inf, -np.inf
    ref = G.int_scatter(x, lut, bad, interpolation)
    gx, glut, got_gmax, got_sums = run(P, x, lut, bad, interpolation)
    assert got_gmax == ref[0] and np.array_equal(got_sums, ref[1]) and np.array_equal(bits(glut), ref[3].view(np.uint32))
    assert torch.isfinite(gx).all() and torch.isfinite(glut).all()
    _, glut, got_gmax, _ = run(P, x, lut, np.full_like(g, np.nan), interpolation)
    assert got_gmax == 0 and not bits(glut).any()
    # 60 decades of magnitudes: the unit follows the largest, the small ones round to nothing, as the bound says
    rs = np.random.RandomState(3)
    wide = (np.sign(rs.randn(*g.shape)) * 10.0 ** rs.uniform(-30, 30, g.shape)).astype(np.float32)
    ref = G.int_scatter(x, lut, wide, interpolation)
    _, glut, got_gmax, got_sums = run(P, x, lut, wide, interpolation)
    assert got_gmax == ref[0] and np.array_equal(got_sums, ref[1]) and np.array_equal(bits(glut), ref[3].view(np.uint32))
    exact = G.backward(x, lut, wide, interpolation)[1]
    err = np.abs(glut.cpu().numpy().astype(np.float64) - exact)
    assert np.all(err <= ref[2] * ref[4] + 2.0 ** -24 * np.abs(exact))
    print(f'N = {n} {interpolation}: |g| from 1e-30 to 1e30: max err {err.max():.3e} against max |glut| {np.abs(exact).max():.3e}')


# ---- gx ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interpolation', INTERPOLATIONS)
@pytest.mark.parametrize('n', [2, 3, 17, 33])
def test_gx_against_the_fp64_reference(P, n, interpolation):
    x, lut = G.gx_image(n, seed=n), R.random_lut(n, n)
    g = np.random.RandomState(n).randn(len(x), 3).astype(np.float32)
    keep = G.gx_comparable(x, lut, interpolation)
    assert 1.0 - keep.mean() <= 0.05
    ref, ref32 = G.backward(x, lut, g, interpolation)[0], G.backward(x, lut, g, interpolation, np.float32)[0]
    eps32 = np.abs(ref - ref32)[keep].max()
    gx = run(P, x.reshape(1, -1, 3), lut, g, interpolation, want_lut=False)[0].cpu().numpy().reshape(-1, 3)
    err = np.abs(gx.astype(np.float64) - ref)[keep].max()
    print(f'N = {n} {interpolation}: gx max err {err:.3e}, eps32 {eps32:.3e}, max |gx| {np.abs(ref).max():.1f}, '
          f'{100 * (1 - keep.mean()):.2f} % not compared')
    assert 0 < eps32 and err <= 4 * eps32
    assert np.isfinite(gx).all()
    assert np.all(gx[~G.input_mask(x)] == 0) and (~G.input_mask(x)).sum() >= 20


# ---- autograd ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interpolation', INTERPOLATIONS)
def test_autograd_equals_the_c_abi_call(P, interpolation):
    x, lut, g = standard(17)
    img, table, up = dev(x).requires_grad_(True), dev(lut).requires_grad_(True), dev(g.reshape(x.shape))
    plain = P.lut_apply(img, table, interpolation)
    assert plain.grad_fn is None and not plain.requires_grad
    out = P.lut_apply(img, table, interpolation, differentiable=True)
    assert out.grad_fn is not None and np.array_equal(bits(out), bits(plain))
    assert np.array_equal(bits(plain), bits(P.lut_apply(dev(x), dev(lut), interpolation)))
    out.backward(up)
    gx, glut = P.lut_apply_backward(dev(x), dev(lut), up, interpolation)
    assert np.array_equal(bits(img.grad), bits(gx)) and np.array_equal(bits(table.grad), bits(glut))
    # only the LUT requires a gradient; a CHW image's view and a weighted sum as the loss
    chw = dev(x).permute(2, 0, 1).contiguous()
    table2 = dev(lut).requires_grad_(True)
    (P.lut_apply(chw.permute(1, 2, 0), table2, interpolation, differentiable=True) * up).sum().backward()
    assert np.array_equal(bits(table2.grad), bits(glut))
    img2 = dev(x).requires_grad_(True)
    (P.lut_apply(img2, dev(lut), interpolation, differentiable=True) * up).sum().backward()
    assert np.array_equal(bits(img2.grad), bits(gx))
    with pytest.raises(ValueError, match='differentiable'):
        P.lut_apply(dev(R.u8_image()), dev(lut), differentiable=True)


# ---- the Adam step ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lam', [0.0, 0.3])
@pytest.mark.parametrize('n', [3, 9])
def test_adam_step_against_the_fp64_reference(P, n, lam):
    rs = np.random.RandomState(n)
    lut0 = (R.identity(n) + 0.1 * rs.randn(n, n, n, 3)).astype(np.float32)
    grads = [(rs.randn(n, n, n, 3) * 10.0 ** rs.uniform(-3, 0)).astype(np.float32) for _ in range(3)]
    state = {t: (lut0.astype(t), np.zeros((n, n, n, 3), t), np.zeros((n, n, n, 3), t)) for t in (np.float64, np.float32)}
    cur, m, v = dev(lut0), torch.zeros(n, n, n, 3, device=DEV), torch.zeros(n, n, n, 3, device=DEV)
    for step, grad in enumerate(grads, 1):
        for t in state:
            state[t] = G.adam_step(*state[t][:1], grad, *state[t][1:], step, 5e-3, lam, dtype=t)
        new = P.lut_adam_step(cur, dev(grad), m, v, step, lr=5e-3, lambda_smooth=lam)
        assert new.data_ptr() != cur.data_ptr()
        cur = new
        for name, got, k in (('lut', cur, 0), ('m', m, 1), ('v', v, 2)):
            eps32 = np.abs(state[np.float64][k] - state[np.float32][k]).max()
            err = np.abs(got.cpu().numpy().astype(np.float64) - state[np.float64][k]).max()
            print(f'N = {n} lambda {lam} step {step}: {name} max err {err:.3e}, eps32 {eps32:.3e}')
            assert 0 < eps32 and err <= 4 * eps32
    if lam:
        # the regulariser's gradient is that of post.lut_smoothness
        t = dev(lut0).requires_grad_(True)
        P.lut_smoothness(t).backward()
        want = G.smoothness_grad(lut0)
        assert np.abs(t.grad.cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()


# ---- lut_refine ---------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def refine_reference(rows, steps):
    img = R.smooth_image(48, 1).astype(np.float32)
    target = G.target_histogram(R.true_map(img), 32)
    img = img[:rows]
    ref = G.refine(R.identity(9), img, target, 32, steps, 5e-3, 0.0, 'trilinear')
    ref32 = G.refine(R.identity(9), img, target, 32, steps, 5e-3, 0.0, 'trilinear', np.float32)
    return img, target, ref, ref32


def test_refine_follows_the_fp64_reference_loop(P):
    """The issue's setup: the 48^2 image, N = 9, h = 32, trilinear, lr 5e-3, lambda 0, 50 steps from the identity."""
    from histogram_classes.RGBuvHistBlock import RGBuvHistBlock
    img, target, (_, ref), (_, ref32) = refine_reference(48, 50)
    assert ref[50] <= 0.6 * ref[0]
    block = RGBuvHistBlock(h=32, device=DEV)
    args = (P.lut_identity(9, DEV), dev(img), dev(target.astype(np.float32)), block)
    kw = dict(steps=50, lr=5e-3, lambda_smooth=0.0, interpolation='trilinear', return_losses=True)
    lut, losses = P.lut_refine(*args, **kw)
    again, losses2 = P.lut_refine(*args, **kw)
    assert np.array_equal(bits(lut), bits(again)) and torch.equal(losses, losses2)
    assert lut.shape == (9, 9, 9, 3) and losses.shape == (51,) and args[0].equal(P.lut_identity(9, DEV))
    got = losses.numpy().astype(np.float64)
    worst = 0.0
    for k in (0, 1, 2, 3, 4, 5, 50):
        dist = abs(ref32[k] - ref[k])
        ratio = abs(got[k] - ref[k]) / dist if dist else float('inf')
        worst = max(worst, ratio)
        print(f'step {k}: GPU {got[k]:.7f}, fp64 reference {ref[k]:.7f}, fp32 reference {ref32[k]:.7f}; |GPU - fp64| / |fp32 - fp64| = {ratio:.2f}')
    print(f'GPU loss {got[0]:.4f} -> {got[50]:.4f} ({got[50] / got[0]:.3f} of the initial loss); largest ratio {worst:.2f}')
    assert got[50] <= 0.6 * got[0]
    assert worst <= 10.0
    assert not isinstance(P.lut_refine(*args, steps=2, lr=5e-3, lambda_smooth=0.05, interpolation='trilinear'), tuple)


def test_refine_honours_a_weight_map(P):
    """Zero weight on the lower half of the image equals refining on the upper half.  The two runs differ in the order of the
    histogram's fp32 sums only; the bar per step is 10 x the largest distance so far between the reference loop in fp32 and in
    fp64 arithmetic on the upper half (an error carried through Adam's normalisation does not shrink when that distance does)."""
    from histogram_classes.RGBuvHistBlock import RGBuvHistBlock
    img, target, (_, ref), (_, ref32) = refine_reference(24, 10)
    full = R.smooth_image(48, 1).astype(np.float32)
    assert np.array_equal(full[:24], img)
    block = RGBuvHistBlock(h=32, device=DEV)
    weight = torch.zeros(48, 48, device=DEV)
    weight[:24] = 1.0
    kw = dict(steps=10, lr=5e-3, lambda_smooth=0.0, interpolation='trilinear', return_losses=True)
    t = dev(target.astype(np.float32))
    lut_w, loss_w = P.lut_refine(P.lut_identity(9, DEV), dev(full), t, block, weight=weight, **kw)
    lut_h, loss_h = P.lut_refine(P.lut_identity(9, DEV), dev(img), t, block, **kw)
    _, loss_all = P.lut_refine(P.lut_identity(9, DEV), dev(full), t, block, **kw)
    bar = 10 * np.maximum.accumulate(np.abs(ref32 - ref))
    diff = np.abs(loss_w.numpy().astype(np.float64) - loss_h.numpy())
    print('weighted against cropped, per step |difference| / bar:', ' '.join(f'{d / b:.2f}' for d, b in zip(diff, bar)))
    print(f'max |LUT difference| {float((lut_w - lut_h).abs().max()):.2e}; the unweighted loss differs by {abs(float(loss_all[0] - loss_w[0])):.3f}')
    assert np.all(diff <= bar)
    assert abs(float(loss_all[0] - loss_w[0])) > 1e-3                       # the map is not ignored
    assert abs(float(loss_h[0]) - ref[0]) <= 10 * abs(ref32[0] - ref[0])


# ---- recoloringTrainer.evaluate ---------------------------------------------------------------------------------------------------
def test_evaluate_post_recoloring_lut_refine(P, tmp_path, monkeypatch):
    torch.manual_seed(0)
    import palette_ref
    from ReHistoGAN.rehistoGAN import recoloringTrainer
    from histogram_classes.RGBuvHistBlock import RGBuvHistBlock
    tr = recoloringTrainer('lutr', str(tmp_path / 'results'), str(tmp_path / 'models'), image_size=64, network_capacity=4,
                           batch_size=1, hist_bin=16, hist_insz=32)
    tr.init_GAN()
    photo = palette_ref.smooth(40, 52).astype(np.float64)              # (H, W, 3) in [0, 1], as evaluate receives it
    img = torch.rand(1, 3, 64, 64, device=DEV)
    h = RGBuvHistBlock(h=16, device=DEV)(torch.rand(1, 3, 32, 32, device=DEV))
    writes = []
    real = P.save_rgb
    monkeypatch.setattr(P, 'save_rgb', lambda a, p: (writes.append(a.clone()), real(a, p)))
    src = torch.from_numpy(np.ascontiguousarray(photo, dtype=np.float32)).to(DEV)
    with torch.no_grad():
        g = tr.evaluate('out_lut', image_batch=img, hist_batch=h, original_image=photo, save_input=False, post_recoloring='lut_refine')
    assert len(writes) == 1 and writes[0].dtype == torch.uint8 and writes[0].shape == (40, 52, 3)
    fitted = P.lut_fit(img[0].permute(1, 2, 0), g[0].permute(1, 2, 0), n=33)
    refined, losses = P.lut_refine(fitted, src, h, tr.histBlock, return_losses=True)
    assert torch.equal(writes[0], P.lut_apply(src, refined, quantize=True))
    assert not torch.equal(writes[0], P.lut_apply(src, fitted, quantize=True))
    print(f'evaluate(lut_refine): Hellinger loss of the working copy {float(losses[0]):.4f} -> {float(losses[-1]):.4f} in {len(losses) - 1} steps')
    assert losses[-1] < losses[0]
