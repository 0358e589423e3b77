"""3D colour LUTs on the GPU (hg_lut_*, include/hg_lut.h; post.lut_apply, lut_fit, lut_splat, lut_solve, lut_bake,
lut_compose; recoloringTrainer.evaluate(post_recoloring='lut')) against the numpy restatement tests/lut_ref.py.

apply    fp32 output: the bar is 4 eps32, eps32 being the largest difference between the reference in fp64 and in fp32
         arithmetic on the same inputs (the rule of tests/test_idt_gpu.py and tests/test_palette_gpu.py).  Quantised output: equal
         to (uint8)(ref * 255) except where ref * 255 lies within 255 x that bar of an integer, where +-1 is allowed; such values
         are at most 1 % of the inputs (asserted).
splat    exact equality: every quantity is an integer.
solve    both sides run the same sequence of fp64 operations and round once to fp32; the sweeps are non-expansive, so a
         difference in the last bits of an fp64 operation stays there and can at most flip the one rounding to fp32: the bar is
         2^-22, one fp32 ulp of an entry in [2, 4) and two of an entry in [1, 2) (displacements cover [-2, 2]).
fit      hg_lut_fit equals splat and solve composed by hand bit for bit; end to end the bar is the solve's plus the apply's (an
         interpolated value is a convex combination of entries).
Every test prints what it measured; the figures recorded in DESIGN.md section 6i come from these prints."""
import ctypes

import numpy as np
import pytest
import torch

import lut_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
SOLVE_BAR = 2.0 ** -22
INTERPOLATIONS = ('tetrahedral', 'trilinear')


@pytest.fixture(scope='module')
def P():
    from histogan_amd import build
    build.build()
    from histogan_amd import post
    return post


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def eps32_of(x, lut, interpolation):
    """(reference in fp64, eps32): never below 2^-24, the rounding of an fp32 output just under 1 -- on a handful of pixels the
    fp32 evaluation can hit the fp64 one exactly, which says nothing about the next handful."""
    ref = R.apply(x, lut, interpolation)
    return ref, max(float(np.abs(ref - R.apply(x, lut, interpolation, np.float32)).max()), 2.0 ** -24)


def check_apply(P, image_t, x, lut, interpolation, what, ref=None, eps32=None):
    """fp32 and quantised output of post.lut_apply on `image_t` against the reference on the same pixels x (M, 3) fp32."""
    if ref is None:
        ref, eps32 = eps32_of(x, lut, interpolation)
    assert 0 < eps32 <= 1e-6
    lut_t = dev(lut)
    got = P.lut_apply(image_t, lut_t, interpolation)
    assert got.dtype == torch.float32 and got.shape == image_t.shape[:2] + (3,) and got.is_contiguous()
    err = float(np.abs(got.cpu().numpy().reshape(-1, 3).astype(np.float64) - ref).max())
    q = P.lut_apply(image_t, lut_t, interpolation, quantize=True)
    assert q.dtype == torch.uint8
    share, off = R.quantized_check(q.cpu().numpy(), x, lut, interpolation, 4 * eps32)
    print(f'{what}: eps32 {eps32:.2e}, kernel error {err:.2e}, band share {share:.4f}, off by one {off}')
    assert err <= 4 * eps32 and share <= 0.01
    return got


# ---- apply: every source form, both interpolations, the LDS and the cached path ---------------------------------------------
@pytest.mark.parametrize('interpolation', INTERPOLATIONS)
@pytest.mark.parametrize('n', [2, 3, 17, 33])
def test_apply_source_forms(P, n, interpolation):
    lut = R.random_lut(n, n)
    img = R.apply_image(n, seed=n)                                       # (37, 29, 3)
    x = img.reshape(-1, 3)
    ref, eps32 = eps32_of(x, lut, interpolation)
    hwc = dev(img)
    a = check_apply(P, hwc, x, lut, interpolation, f'N={n} {interpolation} HWC', ref, eps32)
    chw = dev(img.transpose(2, 0, 1)).permute(1, 2, 0)                   # planar storage, an (H, W, 3) view
    assert not chw.is_contiguous()
    b = check_apply(P, chw, x, lut, interpolation, f'N={n} {interpolation} CHW view', ref, eps32)
    rgba = torch.full((37, 29, 4), float('nan'), device=DEV)             # a pixel stride of 4: read in place
    rgba[..., :3] = hwc
    c = check_apply(P, rgba[..., :3], x, lut, interpolation, f'N={n} {interpolation} RGBA crop', ref, eps32)
    big = torch.full((45, 40, 4), float('nan'), device=DEV)              # rows that do not follow one another
    big[5:42, 3:32, :3] = hwc
    d = check_apply(P, big[5:42, 3:32, :3], x, lut, interpolation, f'N={n} {interpolation} strided crop', ref, eps32)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)  # the forms differ in how pixels are read, in nothing else
    off16 = torch.empty(37 * 29 * 3 + 1, device=DEV)[1:].view(37, 29, 3)  # packed but not 16-byte aligned: the strided reader
    off16.copy_(hwc)
    assert torch.equal(P.lut_apply(off16, dev(lut), interpolation), a)


@pytest.mark.parametrize('interpolation', INTERPOLATIONS)
@pytest.mark.parametrize('n', [3, 17, 33])
def test_apply_uint8_source_all_levels(P, n, interpolation):
    lut = R.random_lut(n, 100 + n)
    u8 = R.u8_image()
    assert all(len(np.unique(u8[..., c])) == 256 for c in range(3))
    x = R.levels(u8).reshape(-1, 3)
    got = check_apply(P, dev(u8), x, lut, interpolation, f'N={n} {interpolation} uint8 source')
    assert torch.equal(got, P.lut_apply(dev(R.levels(u8)), dev(lut), interpolation))      # v / 255 is the fp32 division


def raw_apply(P, src_t, u8_in, n_pix, lut_t, tri, out_t, out_u8, blocks=0):
    P.check(P.lib.hg_lut_apply(src_t.data_ptr(), int(u8_in), n_pix, 3, 1, lut_t.data_ptr(), lut_t.shape[0], tri, out_t.data_ptr(),
                               int(out_u8), blocks, P.raw_stream(DEV)), 'hg_lut_apply')


@pytest.mark.parametrize('n', [17, 33])
def test_apply_pixel_counts_and_padding(P, n):
    """1 pixel, one workgroup's share - 1, exact and + 1, three workgroups; the bytes behind the output stay as they were; a
    forced workgroup count (tiles walked in a loop) gives the same bits."""
    tile = P.lib.hg_lut_apply_tile()
    lut = R.random_lut(n, 7)
    lut_t = dev(lut)
    rs = np.random.RandomState(n)
    counts = [1, 2, 3, 5, tile - 1, tile, tile + 1, 3 * tile - 2]
    assert P.lib.hg_lut_apply_blocks(tile) == 1 and P.lib.hg_lut_apply_blocks(tile + 1) == 2 and P.lib.hg_lut_apply_blocks(3 * tile - 2) == 3
    pad = 64
    for m in counts:
        x = rs.uniform(-0.1, 1.1, (m, 3)).astype(np.float32)
        u8 = rs.randint(0, 256, (m, 3)).astype(np.uint8)
        for tri, interpolation in enumerate(INTERPOLATIONS):
            for u8_in, src, xs in ((0, dev(x), x), (1, dev(u8), R.levels(u8))):
                ref, eps32 = eps32_of(xs, lut, interpolation)
                out = torch.full((3 * m + pad,), -7.25, device=DEV)
                raw_apply(P, src, u8_in, m, lut_t, tri, out, 0)
                assert float(np.abs(out[:3 * m].cpu().numpy().reshape(-1, 3) - ref).max()) <= 4 * eps32
                assert torch.all(out[3 * m:] == -7.25)
                outq = torch.full((3 * m + pad,), 201, dtype=torch.uint8, device=DEV)
                raw_apply(P, src, u8_in, m, lut_t, tri, outq, 1)
                assert R.quantized_check(outq[:3 * m].cpu().numpy(), xs, lut, interpolation, 4 * eps32)[0] <= 0.01
                assert torch.all(outq[3 * m:] == 201)
                if m >= tile:
                    for blocks in (1, 2):
                        again = torch.full((3 * m + pad,), -7.25, device=DEV)
                        raw_apply(P, src, u8_in, m, lut_t, tri, again, 0, blocks=blocks)
                        assert torch.equal(again, out)


@pytest.mark.parametrize('interpolation', INTERPOLATIONS)
def test_apply_identity_affine_and_compose(P, interpolation):
    rs = np.random.RandomState(5)
    img = rs.rand(33, 41, 3).astype(np.float32)
    x = img.reshape(-1, 3)
    for n in (2, 17, 33):
        ident = P.lut_identity(n, DEV)
        assert np.array_equal(ident.cpu().numpy(), R.identity(n).astype(np.float32))
        ref, eps32 = eps32_of(x, R.identity(n).astype(np.float32), interpolation)
        got = P.lut_apply(dev(img), ident, interpolation).cpu().numpy().reshape(-1, 3)
        print(f'identity N={n} {interpolation}: eps32 {eps32:.2e}, |out - ref| {np.abs(got - ref).max():.2e}, |out - in| {np.abs(got - x).max():.2e}')
        assert np.abs(got - ref).max() <= 4 * eps32 and np.abs(got.astype(np.float64) - x).max() <= 4 * eps32
    # an affine map without clipping, baked at N = 2: both interpolations are exact for it
    M = torch.tensor([[0.5, 0.2, 0.1], [0.1, 0.6, 0.1], [0.0, 0.2, 0.7]], device=DEV)
    c = torch.tensor([0.05, 0.1, 0.02], device=DEV)
    baked = P.lut_bake(lambda im: (im @ M.t() + c, 'a tuple keeps its first element'), n=2, device=DEV)
    assert baked.shape == (2, 2, 2, 3)
    want = x.astype(np.float64) @ M.cpu().numpy().astype(np.float64).T + c.cpu().numpy().astype(np.float64)
    ref, eps32 = eps32_of(x, baked.cpu().numpy(), interpolation)
    got = P.lut_apply(dev(img), baked, interpolation).cpu().numpy().reshape(-1, 3)
    print(f'affine N=2 {interpolation}: eps32 {eps32:.2e}, |out - affine| {np.abs(got - want).max():.2e}')
    assert np.abs(got - want).max() <= 4 * eps32 + 2.0 ** -24            # + the rounding of the baked entries themselves
    # compose(identity, L) is L (entries in [0, 1]: a composition ends in lut_apply's clip)
    for n in (5, 17, 33):
        L = rs.rand(n, n, n, 3).astype(np.float32)
        nodes = R.identity(n).astype(np.float32).reshape(-1, 3)
        _, eps32 = eps32_of(nodes, L, interpolation)
        eps32 = max(eps32, 2.0 ** -24)
        comp = P.lut_compose(P.lut_identity(n, DEV), dev(L), interpolation)
        assert comp.shape == (n, n, n, 3)
        print(f'compose N={n} {interpolation}: |compose(identity, L) - L| {np.abs(comp.cpu().numpy() - L).max():.2e}, bar {4 * eps32:.2e}')
        assert np.abs(comp.cpu().numpy().astype(np.float64) - L).max() <= 4 * eps32
    wide = dev(R.random_lut(5, 1))
    assert torch.equal(P.lut_compose(P.lut_identity(5, DEV), wide, interpolation),
                       P.lut_apply(P.lut_identity(5, DEV).view(25, 5, 3), wide, interpolation).view(5, 5, 5, 3))


def test_bake_a_palette_transfer(P):
    """color_transfer_palette returns a tuple; lut_bake keeps the image, and the LUT reproduces the transfer at its nodes."""
    import palette_ref
    img = dev(palette_ref.smooth(24, 24).transpose(2, 0, 1).copy())
    ps, pd = P.paired_palette(img, img.flip(0), k=4, iterations=4)
    n = 9
    lut = P.lut_bake(lambda x: P.color_transfer_palette(x, ps, pd), n=n, device=DEV)
    lattice = P.lut_identity(n, DEV).view(n * n, n, 3)
    direct, _ = P.color_transfer_palette(lattice, ps, pd)
    assert torch.equal(lut.view(n * n, n, 3), direct)
    through = P.lut_apply(lattice, lut)
    assert float((through - direct).abs().max()) <= 4 * 2.0 ** -23       # a node value read back: c0 + f (c1 - c0) with f in {0, 1}


# ---- splat: integers, equal to the reference ----------------------------------------------------------------------------------
def splat_cases():
    rs = np.random.RandomState(11)
    cases = {}
    for n in (2, 3, 9, 17, 33):                                          # 33: global atomics; the others: LDS counters
        node = (np.array([[1, 0, n - 1]], dtype=np.float32) / (n - 1)).reshape(1, 1, 3)
        cases[f'node_N{n}'] = (node, node + np.float32(0.25), None, n)
        centre = ((np.array([[0, n - 2, (n - 1) // 2]], dtype=np.float32) + 0.5) / (n - 1)).reshape(1, 1, 3)
        cases[f'centre_N{n}'] = (centre, centre - np.float32(0.125), None, n)
        s, t = rs.rand(16, 16, 3).astype(np.float32), rs.rand(16, 16, 3).astype(np.float32)
        cases[f'random16_N{n}'] = (s, t, None, n)
    for n in (3, 17, 33):
        s64, t64, _, _ = R.synthetic(2, full=128, small=64)
        w = rs.rand(64, 64).astype(np.float32)
        w[rs.rand(64, 64) < 0.3] = 0.0
        w[0, :5] = [1.0, 2.0, -1.0, np.nan, 0.5]                          # clamped, clamped, clamped to 0, skipped
        cases[f'weighted64_N{n}'] = (s64, t64, w, n)
        lo = min(n - 2, 1)
        one = ((np.array([lo, 0, n - 2]) + rs.rand(20, 20, 3)) / (n - 1)).astype(np.float32)
        cases[f'one_cell_N{n}'] = (one, one[::-1].copy(), None, n)
        s, t = rs.uniform(-0.2, 1.2, (24, 30, 3)).astype(np.float32), rs.uniform(-1.0, 2.0, (24, 30, 3)).astype(np.float32)
        s[0, 0], t[0, 1, 2], t[0, 2, 0] = np.nan, np.inf, -np.inf
        s[1, :3, 0], s[1, :3, 1] = [0.0, 1.0, 1.0], [1.0, 0.0, 1.0]
        t[2, :4] = [[-1, 2, -1], [2, -1, 2], [-5, 5, 0], [3, 3, -3]]     # the last two are clamped to |t - x| <= 2
        cases[f'wide_targets_N{n}'] = (s, t, None, n)
    return cases


SPLAT_CASES = splat_cases()


@pytest.mark.parametrize('name', list(SPLAT_CASES))
def test_splat_equals_the_reference(P, name):
    s, t, w, n = SPLAT_CASES[name]
    want = torch.from_numpy(R.splat(s, t, w, n))
    got = P.lut_splat(dev(s), dev(t), n=n, weight=None if w is None else dev(w))
    assert got.dtype == torch.int64 and got.shape == (n, n, n, 4)
    assert torch.equal(got.cpu()[..., 0], want[..., 0]), 'A'
    assert torch.equal(got.cpu()[..., 1:], want[..., 1:]), 'B'
    assert int(got[..., 0].sum()) == int(R.fixed_point(s, t, w, n)[3].sum()) << 15
    assert torch.equal(P.lut_splat(dev(s), dev(t), n=n, weight=None if w is None else dev(w)), got)     # a second run: the same bits
    if s.shape[0] > 1:
        # planar storage and a forced workgroup count: the same integers; sums handed in are added to
        s_v, t_v = dev(s.transpose(2, 0, 1)).permute(1, 2, 0), dev(t.transpose(2, 0, 1)).permute(1, 2, 0)
        assert torch.equal(P.lut_splat(s_v, t_v, n=n, weight=None if w is None else dev(w), blocks=3), got)
        twice = P.lut_splat(dev(s), dev(t), n=n, weight=None if w is None else dev(w), sums=got.clone())
        assert torch.equal(twice, 2 * got)


def test_splat_refuses_more_than_2_22_pixels_without_a_launch(P):
    s = torch.rand(4, 4, 3, device=DEV)
    sums = torch.zeros(3, 3, 3, 4, dtype=torch.int64, device=DEV)
    rc = P.lib.hg_lut_splat(s.data_ptr(), 3, 1, s.data_ptr(), 3, 1, None, (1 << 22) + 1, 3, sums.data_ptr(), 0, P.raw_stream(DEV))
    torch.cuda.synchronize()
    assert rc == -28 and not sums.any()
    from histogan_amd._lib import HgError
    with pytest.raises(HgError, match='2\\^22'):
        P.check(rc, 'hg_lut_splat')
    assert P.lib.hg_lut_fit(s.data_ptr(), 3, 1, s.data_ptr(), 3, 1, None, (1 << 22) + 1, 3, 0.2, 4, sums.data_ptr(), sums.data_ptr(),
                            1 << 30, P.raw_stream(DEV)) == -28


# ---- solve: the reference's sequence on handed-in integers ------------------------------------------------------------------------
def solve_cases(n):
    rs = np.random.RandomState(n)
    shape = (n, n, n)
    zero = np.zeros(shape + (4,), dtype=np.int64)
    single = zero.copy()
    single[n // 2, 0, n - 1] = [12345, 12345 * (1 << 14), -12345 * (1 << 15), 12345 * 3]
    A = rs.randint(1, 1 << 30, shape).astype(np.int64)
    qd = rs.randint(-(1 << 17), (1 << 17) + 1, shape + (3,)).astype(np.int64)
    dense = np.concatenate([A[..., None], A[..., None] * qd], axis=-1)
    sparse = dense * (rs.rand(*shape) < 0.08)[..., None]
    return {'zero': zero, 'single': single, 'sparse': sparse, 'dense': dense}


@pytest.mark.parametrize('n', [3, 9, 17, 33])                            # 33: d in global memory; the others: in LDS
def test_solve_equals_the_reference_sequence(P, n):
    for name, sums in solve_cases(n).items():
        for lam, sweeps in ((0.2, 24), (0.01, 7), (0.0, 2)) if name != 'single' else ((0.2, 40),):
            want = R.solve(sums, lam, sweeps)
            got = P.lut_solve(dev(sums), lambda_smooth=lam, iterations=sweeps)
            assert got.dtype == torch.float32 and got.shape == (n, n, n, 3)
            err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
            same = bool(np.array_equal(got.cpu().numpy(), want))
            print(f'solve N={n} {name} lambda {lam} sweeps {sweeps}: max |gpu - ref| {err:.2e} (bar {SOLVE_BAR:.2e}), equal bits: {same}')
            assert err <= SOLVE_BAR
            assert torch.equal(P.lut_solve(dev(sums), lambda_smooth=lam, iterations=sweeps), got)       # a second run
            if name == 'zero':
                assert np.array_equal(got.cpu().numpy(), R.identity(n).astype(np.float32))
    # a single node with data: converged, the displacement is the constant b / a at every node
    if n == 3:
        sums = solve_cases(n)['single']
        got = P.lut_solve(dev(sums), lambda_smooth=0.2, iterations=3000).cpu().numpy().astype(np.float64)
        d = got - R.identity(n)
        assert np.abs(d - np.array([2.0 ** 14, -2.0 ** 15, 3.0]) / 2.0 ** 16).max() <= SOLVE_BAR
    # the defaults
    sums = solve_cases(n)['sparse']
    assert np.abs(P.lut_solve(dev(sums)).cpu().numpy().astype(np.float64) - R.solve(sums)).max() <= SOLVE_BAR


# ---- fit ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def PAIR():
    s64, t64, _, _ = R.synthetic(0)
    return s64, t64


@pytest.mark.parametrize('n', [9, 17, 33])
def test_fit_equals_splat_and_solve_composed_by_hand(P, PAIR, n):
    s, t = dev(PAIR[0]), dev(PAIR[1])
    w = dev(np.random.RandomState(n).rand(64, 64).astype(np.float32))
    for weight in (None, w):
        for lam, sweeps in ((None, None), (0.05, 10)):
            fit = P.lut_fit(s, t, n=n, weight=weight, lambda_smooth=lam, iterations=sweeps)
            by_hand = P.lut_solve(P.lut_splat(s, t, n=n, weight=weight), lambda_smooth=lam, iterations=sweeps)
            assert torch.equal(fit, by_hand)
    chw_s, chw_t = dev(PAIR[0].transpose(2, 0, 1)).permute(1, 2, 0), dev(PAIR[1].transpose(2, 0, 1)).permute(1, 2, 0)
    assert torch.equal(P.lut_fit(chw_s, chw_t, n=n), P.lut_fit(s, t, n=n))


def test_fit_of_an_image_to_itself_is_the_identity(P, PAIR):
    s = dev(PAIR[0])
    for n in (2, 17, 33):
        lut = P.lut_fit(s, s, n=n)
        assert torch.equal(lut, P.lut_identity(n, DEV))
        for interpolation in INTERPOLATIONS:
            ref, eps32 = eps32_of(PAIR[0].reshape(-1, 3), R.identity(n).astype(np.float32), interpolation)
            got = P.lut_apply(s, lut, interpolation).cpu().numpy().reshape(-1, 3).astype(np.float64)
            assert np.abs(got - PAIR[0].reshape(-1, 3)).max() <= 4 * eps32
    # without any weight there is no data: the identity as well, with no read-back and no error
    assert torch.equal(P.lut_fit(s, dev(PAIR[1]), n=9, weight=torch.zeros(64, 64, device=DEV)), P.lut_identity(9, DEV))


@pytest.mark.parametrize('n', [17, 33])
def test_fit_and_apply_end_to_end(P, PAIR, n):
    s64, t64 = PAIR
    x = s64.reshape(-1, 3)
    ref_lut = R.fit(s64, t64, None, n)
    lut = P.lut_fit(dev(s64), dev(t64), n=n)
    e_lut = float(np.abs(lut.cpu().numpy().astype(np.float64) - ref_lut).max())
    for interpolation in INTERPOLATIONS:
        ref, eps32 = eps32_of(x, ref_lut, interpolation)
        got = P.lut_apply(dev(s64), lut, interpolation).cpu().numpy().reshape(-1, 3)
        err = float(np.abs(got - ref).max())
        fidelity = float(np.abs(got - np.clip(t64.reshape(-1, 3), 0, 1)).mean())
        print(f'end to end N={n} {interpolation}: max |lut - ref| {e_lut:.2e}, max |apply - ref| {err:.2e} '
              f'(bar {4 * eps32 + SOLVE_BAR:.2e}), mean |apply(fit)(s) - t| {fidelity:.2e}')
        assert e_lut <= SOLVE_BAR and err <= 4 * eps32 + SOLVE_BAR


# ---- recoloringTrainer.evaluate ---------------------------------------------------------------------------------------------------
def test_evaluate_post_recoloring_lut(P, tmp_path, monkeypatch):
    torch.manual_seed(0)
    import palette_ref
    from ReHistoGAN.rehistoGAN import recoloringTrainer
    from histogram_classes.RGBuvHistBlock import RGBuvHistBlock
    tr = recoloringTrainer('lut', str(tmp_path / 'results'), str(tmp_path / 'models'), image_size=64, network_capacity=4,
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
        g = tr.evaluate('out_lut', image_batch=img, hist_batch=h, original_image=photo, save_input=False, post_recoloring='lut')
    assert len(writes) == 1 and writes[0].dtype == torch.uint8 and writes[0].shape == (40, 52, 3)
    lut = P.lut_fit(img[0].permute(1, 2, 0), g[0].permute(1, 2, 0), n=33)
    assert torch.equal(writes[0], P.lut_apply(src, lut, quantize=True))
    assert not torch.equal(writes[0], P.color_transfer_mkl(src, g[0].permute(1, 2, 0), quantize=True)[0])
    # the file a user would exchange: the same LUT through save_cube / load_cube applies to the same bytes
    back = P.load_cube(P.save_cube(lut, str(tmp_path / 'look.cube'), title='lut'), device=DEV)
    assert torch.equal(back, lut) and torch.equal(P.lut_apply(src, back, quantize=True), writes[0])
    with pytest.raises(ValueError, match='batch of one'):
        tr.evaluate('two', image_batch=torch.rand(2, 3, 64, 64, device=DEV), hist_batch=torch.cat([h, h]), original_image=photo,
                    post_recoloring='lut')
    with pytest.raises(ValueError, match='post_recoloring'):
        tr.evaluate('bad', image_batch=img, hist_batch=h, original_image=photo, post_recoloring='nonsense')
