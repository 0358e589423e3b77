"""CPU-side checks of the palette (hg_palette_*, include/hg_post.h; post.palette, paired_palette, palette_labels,
match_palettes, color_transfer_palette, palette_histogram; recoloringTrainer.evaluate(post_recoloring='palette')): the
integer reference of tests/palette_ref.py against the invariants its definition promises, and the host side of the C ABI and
of the Python surface.  No kernel is launched.

Before the feature the ABI tests fail for want of the symbols and of version 114, and the Python-surface tests for want of
the functions and of evaluate's third mode."""
import ctypes
import types

import numpy as np
import pytest
import torch

import palette_ref as R
import post_ref

EINVAL, EWORKSPACE, EK, EPIXELS = -1, -4, -25, -26


@pytest.fixture(scope='module')
def L():
    from histogan_amd import build
    build.build()
    import histogan_amd._lib as L
    return L


# ---- the reference's own invariants --------------------------------------------------------------------------------------
def test_reference_conversions_round_trip_and_agree():
    rgb = np.random.RandomState(0).rand(500, 3).astype(np.float32)
    lab = R.srgb_to_lab(rgb)
    assert np.abs(R.lab_to_srgb(lab) - rgb).max() <= 1e-12
    assert np.abs(lab - R.srgb_to_lab(rgb, root='pow')).max() <= 1e-12
    white = R.srgb_to_lab(np.ones((1, 3), dtype=np.float32))[0]
    assert abs(white[0] - 100.0) <= 1e-12 and np.abs(white[1:]).max() <= 1e-12
    assert np.abs(np.rint(R.UNIT * lab)).max() < 2 ** 14               # the gamut in units of 1/128


def test_weights_add_up_and_a_lloyd_step_never_raises_the_cost():
    px, _ = R.clustered(K=5, per_blob=120, seed=1, spread=0.05)
    w = np.random.RandomState(1).rand(len(px)).astype(np.float32)
    w[::7] = 0.0
    px[3] = np.nan
    pts = R.quantize(px, w)
    assert pts[3, 3] == 0 and np.all(pts[::7, 3] == 0) and not pts[3, :3].any()
    cells = R.bins(pts)
    total = int(pts[:, 3].sum())
    assert int(cells[:, 0].sum()) == total
    for K in (1, 3, 8):
        c = R.seeds(cells, K)
        costs = [R.cost(pts, c)]
        for _ in range(6):
            s, lab = R.step(pts, pts, c)
            assert int(s[:, 0].sum()) == total and np.all(lab[pts[:, 3] == 0] == R.NO_LABEL)
            c = R.update(s, c)
            costs.append(R.cost(pts, c))
        # cost(c) = cost(mean) + W |c - mean|^2 per cluster, and the rounded mean is the integer point nearest the mean: no
        # integer centre, the old one included, has a lower cost -- so not even the rounding can raise it
        assert all(b <= a for a, b in zip(costs, costs[1:])), costs
        assert costs[-1] < costs[0] or K == 1


def test_floor_mean_rounds_halves_up_also_below_zero():
    assert [int(R.floor_mean(np.int64(s), np.int64(2))) for s in (-3, -2, -1, 0, 1, 2, 3)] == [-1, -1, 0, 0, 1, 1, 2]
    sums = np.array([[2, 10, -3, -5], [0, 99, 99, 99]], dtype=np.int64)
    assert R.update(sums, np.array([[7, 7, 7], [1, 2, 3]])).tolist() == [[5, -1, -2], [1, 2, 3]]     # the empty cluster keeps its centre


@pytest.mark.parametrize('K', [2, 6, 16])
def test_clustered_recovers_its_blobs(K):
    px, blob = R.clustered(K=K, per_blob=60, seed=K)
    pts = R.quantize(px)
    c, sums, labels, _ = R.run(pts, K, 8)
    table = {(int(a), int(b)) for a, b in zip(blob, labels)}
    assert len(table) == K and len({a for a, _ in table}) == K and len({b for _, b in table}) == K      # one to one
    want = np.stack([R.srgb_to_lab(px[blob == k]).mean(axis=0) for k in range(K)])
    got = {b: a for a, b in table}
    for k in range(K):
        assert np.abs(c[k] / R.UNIT - want[got[k]]).max() <= 0.05


def test_seeds_duplicate_when_all_weight_sits_in_one_cell_and_ties_take_the_lowest_index():
    pts = np.array([[5000, 100, 100, 9], [5010, 120, 90, 3]], dtype=np.int64)
    assert len(set(R.cell_of(pts))) == 1
    s = R.seeds(R.bins(pts), 4)
    assert np.all(s == s[0]) and s[0].tolist() == R.floor_mean(R.bins(pts)[R.cell_of(pts)[0], 1:], np.int64(12)).tolist()
    assert not R.seeds(R.bins(np.zeros((3, 4), dtype=np.int64)), 3).any()
    tp, tc = R.ties()
    d = R.distances(tp, tc)
    tied = d[:, 0] == d[:, 1]
    assert tied.sum() >= len(tp) // 2 and (~tied).sum() >= len(tp) // 4
    _, lab = R.step(tp, tp, tc)
    assert np.all(lab[tied] == 0) and set(lab[~tied]) == {0, 1}


def test_paired_palette_of_an_image_with_itself_is_the_palette():
    px = R.smooth().reshape(-1, 3)
    pts = R.quantize(px)
    for iters in (0, 2, 5):                                        # converged or not: both are means over the same clusters
        c, sums, _, other = R.run(pts, 6, iters, value=pts)
        assert np.array_equal(other, c)


def test_palette_transfer_beats_the_affine_map_on_per_blob_shifts():
    """The property tests/test_palette_gpu.py relies on, on the reference alone: blobs that each move by their own Lab offset are
    followed by the palette transfer with a sigma that separates them (palette_ref.separating_sigma: chosen from the geometry of
    the centres, not from the result) and not by one affine map.  The default sigma, the mean distance between the centres, is
    far smoother -- it blends every shift into every pixel -- and is printed for comparison only."""
    K = 6
    px, blob = R.clustered(K=K, per_blob=150, seed=2)
    tgt = R.shifted(px, blob, K, seed=2)
    pts, pts_t = R.quantize(px), R.quantize(tgt)
    c, sums, _, other = R.run(pts, K, 8, value=pts_t)
    live = sums[:, 0] > 0
    out, sigma = R.transfer(px, c / R.UNIT, other / R.UNIT, live=live, sigma=R.separating_sigma(c / R.UNIT, live))
    smooth, sigma0 = R.transfer(px, c / R.UNIT, other / R.UNIT, live=live)
    mkl, _ = post_ref.color_transfer(px.reshape(-1, 1, 3), tgt.reshape(-1, 1, 3))
    e_pal, e_mkl = np.abs(out - tgt).mean(), np.abs(mkl.reshape(-1, 3) - tgt).mean()
    print(f'per-blob shifts, mean |out - shifted|: palette transfer {e_pal:.2e} (sigma {sigma:.2f}), MKL {e_mkl:.2e}; with the '
          f'default sigma {sigma0:.2f}: {np.abs(smooth - tgt).mean():.2e}')
    assert e_pal < e_mkl


def test_transfer_reference_identity_and_translation():
    px, lab, _, _, _ = R.transfer_case('identity')
    same, _ = R.transfer(px, lab, lab)
    assert np.abs(same - px).max() <= 1e-12
    one, sg = R.transfer(px, lab[:1], lab[:1] + np.float32([2.0, -3.0, 1.0]))
    assert sg == 1.0 and np.abs(R.srgb_to_lab(one) - R.srgb_to_lab(px) - [2.0, -3.0, 1.0]).max() <= 1e-9    # in gamut: a translation
    assert R.default_sigma(lab, np.ones(6, bool)) > 1.0 and R.default_sigma(lab, np.arange(6) == 3) == 1.0
    assert R.default_sigma(np.zeros((4, 3), np.float32), np.ones(4, bool)) == 1.0                          # a mean of 0 takes 1


@pytest.mark.parametrize('name', R.TRANSFER_CASES)
def test_transfer_cases_are_well_conditioned(name):
    """The inputs of tests/test_palette_gpu.py's transfer cases: the fp32 and the fp64 reference agree to 1e-5, and their
    quantised outputs differ by one 8-bit level on at most 0.1 % of the values -- the caps the kernel is then held to."""
    px, src, dst, live, sigma = R.transfer_case(name)
    a, sg = R.transfer(px, src, dst, live, sigma)
    b, _ = R.transfer(px, src, dst, live, sigma, dtype=np.float32)
    eps32 = float(np.abs(a - b).max())
    q = np.abs(R.to_u8(a).astype(int) - R.to_u8(b).astype(int))
    print(f'transfer ({name}, sigma {sg:.2f}): eps32 {eps32:.2e}; 8-bit values that differ {int((q > 0).sum())} of {q.size}')
    assert eps32 <= 1e-5 and q.max() <= 1 and (q > 0).sum() <= q.size // 1000
    assert 0.0 < a.min() and a.max() < 1.0 or name != 'identity'


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def test_exports_and_version(L):
    names = ('max_k', 'blocks', 'point_stride', 'workspace_bytes', 'quantize', 'bins', 'seeds', 'step', 'update', 'run', 'transfer')
    for n in names:
        assert 'hg_palette_' + n in L.EXPORTS and getattr(L.lib, 'hg_palette_' + n).argtypes is not None
    assert L.lib.hg_version() >= 114
    assert b'palette' in L.lib.hg_error_string(EK) and b'palette' in L.lib.hg_error_string(EPIXELS)
    assert L.lib.hg_palette_max_k() == R.MAX_K


def test_plan_queries(L):
    lib = L.lib
    assert lib.hg_palette_blocks(1) == 1 and lib.hg_palette_blocks(0) == 0 and lib.hg_palette_blocks(2 ** 28) == 0
    assert lib.hg_palette_blocks(2 ** 28 - 1) >= 1
    assert [lib.hg_palette_point_stride(n) for n in (0, 1, 2, 63, 2 ** 28 - 1, 2 ** 28)] == [0, 2, 2, 64, 2 ** 28, 0]
    b = [lib.hg_palette_blocks(n) for n in (1, 1000, 10 ** 5, 10 ** 7, 2 ** 28 - 1)]
    assert b == sorted(b) and b[0] == 1 and b[2] > 1 and b[-1] == b[-2]                   # grows, then capped
    q = lib.hg_palette_workspace_bytes
    up16 = lambda v: (v + 15) // 16 * 16                                                  # noqa: E731
    cells = R.CELLS * 4 * 8
    assert q(1, 63, 0) == up16(64 * 8) + cells
    assert q(3, 63, 1) == 2 * up16(3 * 64 * 8) + 3 * cells + up16(3 * R.MAX_K * 4 * 8)
    assert q(0, 63, 0) == 0 and q(65536, 63, 0) == 0 and q(1, 0, 0) == 0 and q(1, 2 ** 28, 0) == 0


def test_every_refusal_has_its_code_and_nothing_is_launched(L):
    """The library loads without a GPU; every call below returns before it would launch, so the pointers -- never
    dereferenced on the host -- need not be real."""
    lib = L.lib
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    big = 2 ** 28
    quant = lambda x=p, pts=p, B=1, H=4, W=5: lib.hg_palette_quantize(x, 20, 1, 5, 1, None, 0, 0, 0, pts, B, H, W, None)   # noqa: E731
    assert quant(x=None) == EINVAL and quant(pts=None) == EINVAL and quant(pts=odd) == EINVAL and quant(B=0) == EINVAL
    assert quant(H=0) == EINVAL and quant(H=2 ** 14, W=2 ** 14) == EPIXELS
    bins = lambda pts=p, B=1, n=10, b=p, blocks=0: lib.hg_palette_bins(pts, B, n, b, blocks, None)                          # noqa: E731
    assert bins(pts=None) == EINVAL and bins(b=None) == EINVAL and bins(pts=odd) == EINVAL and bins(blocks=-1) == EINVAL
    assert bins(blocks=4096) == EINVAL and bins(n=0) == EPIXELS and bins(n=big) == EPIXELS and bins(B=0) == EINVAL
    seeds = lambda b=p, B=1, K=4, c=p: lib.hg_palette_seeds(b, B, K, c, None)                                               # noqa: E731
    assert seeds(b=None) == EINVAL and seeds(c=None) == EINVAL and seeds(K=0) == EK and seeds(K=17) == EK
    step = lambda a=p, v=p, B=1, n=10, c=p, K=4, s=p, lab=None, blocks=0: lib.hg_palette_step(a, v, B, n, c, K, s, lab, blocks, None)  # noqa: E731
    assert step(a=None) == EINVAL and step(v=None) == EINVAL and step(c=None) == EINVAL and step(s=None) == EINVAL
    assert step(a=odd) == EINVAL and step(K=0) == EK and step(K=17) == EK and step(n=0) == EPIXELS and step(n=big) == EPIXELS
    upd = lambda s=p, B=1, K=4, c=p: lib.hg_palette_update(s, B, K, c, 1, None)                                             # noqa: E731
    assert upd(s=None) == EINVAL and upd(c=None) == EINVAL and upd(K=0) == EK and upd(K=17) == EK
    ws = lib.hg_palette_workspace_bytes(1, 20, 1)

    def run(x=p, other=None, H=4, W=5, K=4, iters=3, blocks=0, c=p, s=p, co=None, wsp=p, nbytes=ws):
        return lib.hg_palette_run(x, 20, 1, 5, 1, None, 0, 0, 0, other, 20, 1, 5, 1, 1, H, W, K, iters, blocks, c, s, co, None, wsp,
                                  nbytes, None)
    for kw in (dict(x=None), dict(c=None), dict(s=None), dict(wsp=None), dict(wsp=odd), dict(iters=-1), dict(blocks=-1),
               dict(other=p), dict(co=p), dict(W=0)):
        assert run(**kw) == EINVAL, kw
    assert run(K=0) == EK and run(K=17) == EK and run(H=2 ** 14, W=2 ** 14, nbytes=1 << 60) == EPIXELS
    assert run(nbytes=lib.hg_palette_workspace_bytes(1, 20, 0) - 1) == EWORKSPACE
    assert run(other=p, co=p, nbytes=ws - 1) == EWORKSPACE and run(nbytes=0) == EWORKSPACE

    def tr(x=p, n=10, ps=3, cs=1, s=p, d=p, live=p, K=4, sigma=0.0, su=p, out=p, u8=0):
        return lib.hg_palette_transfer(x, n, ps, cs, s, d, live, K, sigma, su, out, u8, None)
    for kw in (dict(x=None), dict(s=None), dict(d=None), dict(live=None), dict(su=None), dict(out=None), dict(out=odd), dict(ps=0),
               dict(cs=-1), dict(sigma=float('nan')), dict(sigma=float('inf'))):
        assert tr(**kw) == EINVAL, kw
    assert tr(K=0) == EK and tr(K=17) == EK and tr(n=0) == EPIXELS and tr(n=big) == EPIXELS


# ---- the Python surface refuses before a device is touched ----------------------------------------------------------------
def test_python_surface_value_errors_and_cpu_refusal(L):
    from histogan_amd import post
    img = torch.rand(3, 8, 9)
    for kw, word in ((dict(k=0), 'k must'), (dict(k=17), 'k must'), (dict(k=2.0), 'k must'), (dict(iterations=-1), 'iterations'),
                     (dict(weight=torch.rand(8, 8)), 'weight must')):
        with pytest.raises(ValueError, match=word):
            post.palette(img, **kw)
    with pytest.raises(ValueError, match='float'):
        post.palette(torch.zeros(3, 8, 9, dtype=torch.uint8))
    with pytest.raises(ValueError, match='one shape'):
        post.paired_palette(img, torch.rand(3, 8, 8))
    with pytest.raises(RuntimeError, match='palette.*no CPU implementation'):
        post.palette(img)
    with pytest.raises(RuntimeError, match='paired_palette.*no CPU implementation'):
        post.paired_palette(img, img)
    pal = post.Palette(torch.rand(4, 3), torch.rand(4, 3) * 50, torch.full((4,), 0.25))
    assert pal._fields == ('rgb', 'lab', 'weight')
    with pytest.raises(RuntimeError, match='palette_labels.*no CPU implementation'):
        post.palette_labels(img, pal)
    with pytest.raises(ValueError, match='palette_labels'):
        post.palette_labels(img, torch.rand(4, 2))
    with pytest.raises(RuntimeError, match='match_palettes.*no CPU implementation'):
        post.match_palettes(pal, pal)
    with pytest.raises(ValueError, match="by must be 'lightness'"):
        post.match_palettes(pal, pal, by='hue')
    other = post.Palette(torch.rand(5, 3), torch.rand(5, 3), torch.full((5,), 0.2))
    with pytest.raises(ValueError, match='one K'):
        post.match_palettes(pal, other)
    src = torch.rand(8, 9, 3)
    with pytest.raises(ValueError, match='one K'):
        post.color_transfer_palette(src, pal, other)
    with pytest.raises(ValueError, match='src_palette must be a Palette'):
        post.color_transfer_palette(src, torch.rand(4, 3), pal)
    for bad in (0.0, -1.0, float('nan'), float('inf'), 'wide'):
        with pytest.raises(ValueError, match='sigma'):
            post.color_transfer_palette(src, pal, pal, sigma=bad)
    with pytest.raises(ValueError, match=r'source must be an \(H, W, 3\) image'):
        post.color_transfer_palette(torch.rand(8, 9, 4), pal, pal)
    with pytest.raises(RuntimeError, match='color_transfer_palette.*no CPU implementation'):
        post.color_transfer_palette(src, pal, pal)
    with pytest.raises(ValueError, match='palette_histogram'):
        post.palette_histogram(lambda x, weight=None: x, torch.rand(4, 3))
    with pytest.raises(RuntimeError, match='palette_histogram.*no CPU implementation'):
        post.palette_histogram(lambda x, weight=None: x, pal)
    assert 'palette' in post.__doc__ and 'third transfer' in post.__doc__


def test_evaluate_names_all_three_modes(L):
    from histogan_amd import project
    from histogan_amd.retrainer import recoloringTrainer
    for bad in ('nonsense', 'Palette', 'mkl', ''):
        with pytest.raises(ValueError, match="post_recoloring=.*'idt'.*'palette'") as e:
            recoloringTrainer.evaluate(types.SimpleNamespace(), post_recoloring=bad)
        assert 'Monge-Kantorovich' in str(e.value)
    assert 'color_transfer_palette' in project.__doc__ and 'third transfer' in project.__doc__
