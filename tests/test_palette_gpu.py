"""The palette on the GPU (hg_palette_*, include/hg_post.h; post.palette, paired_palette, palette_labels, match_palettes,
color_transfer_palette, palette_histogram; recoloringTrainer.evaluate(post_recoloring='palette')) against the numpy restatement
tests/palette_ref.py.

quantise   |q - q_ref| <= 1 and at most n / 1000 values differ (a 1-ulp difference between two fp64 evaluations of the chain can
           flip one rint; two formulations of the reference stay within the same cap of each other); weights, non-finite pixels
           and padding are exact.
bins, seeds, step, update, run   exact equality: every quantity is an integer.
transfer   the bar is 4 eps32, eps32 being the largest difference between the reference in fp64 and in fp32 arithmetic on the
           same inputs; a case whose eps32 exceeds 1e-5 fails as ill-conditioned (the rule of tests/test_idt_gpu.py).  The
           quantised output may differ from the reference's by one 8-bit level on at most 0.1 % of the values.
Measured on the MI355X (41 x 51 photo, 2091 pixels):

    case             sigma   eps32     kernel error
    one_colour        1.00   2.50e-06  2.98e-08
    default_sigma    48.54   3.84e-06  2.98e-08
    explicit_sigma    6.50   2.80e-06  2.98e-08
    separating        6.27   2.89e-06  2.98e-08
    not_live         47.35   1.49e-06  2.98e-08
    identity         48.54   1.06e-06  9.71e-16
    strided          48.54   3.84e-06  2.98e-08

(2.98e-08 is half an ulp of the fp32 output: the kernel evaluates in fp64 and rounds once.)  No quantised value differed from
the reference's, and no quantised point: every integer stage, hg_palette_run against the stages composed by hand, a second
run, a run with one workgroup per image and the reference are equal bit for bit."""
import numpy as np
import pytest
import torch

import palette_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)


@pytest.fixture(scope='module')
def P():
    from histogan_amd import build
    build.build()
    from histogan_amd import post
    return post


@pytest.fixture(scope='module')
def SHARE(P):
    """The largest point count one workgroup takes, from the exported plan (doubling, then bisecting)."""
    lib = P.lib
    n = 1
    while lib.hg_palette_blocks(n + 1) == 1:
        n *= 2
    lo, hi = n // 2, n + 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lib.hg_palette_blocks(mid) == 1 else (lo, mid)
    assert lib.hg_palette_blocks(lo) == 1 and lib.hg_palette_blocks(lo + 1) == 2
    return lo


# ---- plumbing: the stage entry points on torch tensors -----------------------------------------------------------------
def stream(P):
    return P.raw_stream(DEV)


def random_points(n, seed, extremes=True):
    """int64 (n, 4) handed-in points: mostly in gamut, weights with zeros, and -- the cell clamps -- a few at the ends of int16."""
    rs = np.random.RandomState(seed)
    pts = np.stack([rs.randint(0, 12801, n), rs.randint(-12000, 12001, n), rs.randint(-12000, 12001, n), rs.randint(0, 65536, n)],
                   axis=1).astype(np.int64)
    pts[rs.rand(n) < 0.1, 3] = 0
    if extremes and n >= 8:
        pts[1, :3] = (-5, -32768, 32767)
        pts[2, :3] = (32767, 32767, -32768)
        pts[3, 3] = 65535
    return pts


def dev_points(P, batches):
    """int16 (B, stride, 4) device tensor of B point sets of one length; the padding has qw = 0, as the contract asks, and
    coordinates that would show if they were used."""
    n = len(batches[0])
    stride = P.lib.hg_palette_point_stride(n)
    assert stride >= n and stride % 2 == 0 and stride - n < 2
    buf = np.zeros((len(batches), stride, 4), dtype=np.int64)
    buf[:, n:, :3] = 12345
    for b, pts in enumerate(batches):
        buf[b, :n] = pts
    as16 = np.concatenate([buf[..., :3].astype(np.int16), buf[..., 3:].astype(np.uint16).view(np.int16)], axis=-1)
    return torch.from_numpy(np.ascontiguousarray(as16)).to(DEV)


def host_points(t, n):
    """int64 (B, n, 4) of a device point tensor."""
    a = t.cpu().numpy()
    return np.concatenate([a[:, :n, :3].astype(np.int64), a[:, :n, 3:].view(np.uint16).astype(np.int64)], axis=-1)


def gpu_bins(P, pts_t, B, n, blocks=0):
    out = torch.zeros((B, R.CELLS, 4), dtype=torch.int64, device=DEV)
    P.check(P.lib.hg_palette_bins(pts_t.data_ptr(), B, n, out.data_ptr(), blocks, stream(P)), 'hg_palette_bins')
    return out


def gpu_seeds(P, bins_t, B, K):
    out = torch.full((B, K, 3), -777, dtype=torch.int32, device=DEV)
    P.check(P.lib.hg_palette_seeds(bins_t.data_ptr(), B, K, out.data_ptr(), stream(P)), 'hg_palette_seeds')
    return out


def gpu_step(P, assign_t, value_t, B, n, centres, K, blocks=0, start=None, labels=True):
    c_t = centres if torch.is_tensor(centres) else torch.from_numpy(np.asarray(centres, dtype=np.int32).reshape(B, K, 3)).to(DEV)
    sums = torch.zeros((B, K, 4), dtype=torch.int64, device=DEV) if start is None else start.clone()
    lab = torch.full((B, n), 77, dtype=torch.uint8, device=DEV) if labels else None
    P.check(P.lib.hg_palette_step(assign_t.data_ptr(), value_t.data_ptr(), B, n, c_t.data_ptr(), K, sums.data_ptr(), P.ptr(lab),
                                  blocks, stream(P)), 'hg_palette_step')
    return sums, lab


def gpu_update(P, sums_t, centres_t, clear):
    B, K, _ = centres_t.shape
    P.check(P.lib.hg_palette_update(sums_t.data_ptr(), B, K, centres_t.data_ptr(), int(clear), stream(P)), 'hg_palette_update')


def sizes(SHARE):
    return {'one': 1, 'share-1': SHARE - 1, 'share': SHARE, 'share+1': SHARE + 1, 'three_workgroups': 2 * SHARE + 1027}


SIZE_NAMES = ['one', 'share-1', 'share', 'share+1', 'three_workgroups']


# ---- quantise --------------------------------------------------------------------------------------------------------------
def quantise_case(name):
    """(image (B, 3, H, W) view, weight (B, H, W) or None)."""
    rs = np.random.RandomState(11)
    if name == 'small':                                   # 63 pixels: an odd count, a weight map with zeros, bad pixels
        img = torch.from_numpy(rs.uniform(-0.2, 1.2, (1, 3, 7, 9)).astype(np.float32))
        img[0, 0, 0, 1], img[0, 2, 3, 3], img[0, 1, 6, 8] = float('nan'), float('inf'), float('-inf')
        w = torch.from_numpy(rs.uniform(-0.3, 1.3, (1, 7, 9)).astype(np.float32))
        w[0, 2, :4] = 0.0
        w[0, 5, 5] = float('nan')
        return img, w
    if name == 'strided_batch':                           # B = 2, a view with strides in every dimension, 143 pixels
        base = torch.from_numpy(rs.uniform(0, 1, (3, 4, 11, 26)).astype(np.float32))
        return base[:2, 1:, :, ::2], None
    base = torch.from_numpy(rs.uniform(-0.1, 1.1, (1, 37, 41, 3)).astype(np.float32))      # HWC storage, three workgroups
    return base.permute(0, 3, 1, 2), torch.from_numpy(rs.rand(1, 1, 37, 41).astype(np.float32))[:, 0]


@pytest.mark.parametrize('name', ['small', 'strided_batch', 'channels_last'])
def test_quantise_against_fp64(P, name):
    img, w = quantise_case(name)
    B, _, H, W = img.shape
    n = H * W
    assert {'small': n % 2 == 1 and img.shape[1:] == (3, 7, 9), 'strided_batch': B == 2 and not img.is_contiguous() and n % 2 == 1,
            'channels_last': img.stride(1) == 1 and n > 2 * 512}[name]
    x = img.to(DEV) if img.is_contiguous() else torch.empty_strided(img.shape, img.stride(), device=DEV).copy_(img)
    assert x.stride() == img.stride()
    wd = None if w is None else w.to(DEV)
    stride = P.lib.hg_palette_point_stride(n)
    pts = torch.full((B, stride, 4), 0x7f7f, dtype=torch.int16, device=DEV)                 # garbage: the padding must be written
    P.check(P.lib.hg_palette_quantize(x.data_ptr(), *x.stride(), P.ptr(wd), *((0, 0, 0) if wd is None else wd.stride()),
                                      pts.data_ptr(), B, H, W, stream(P)), 'hg_palette_quantize')
    raw = pts.cpu().numpy()
    assert not raw[:, n:].any()                                                             # padding: qw = 0, coordinates 0
    got = host_points(pts, n)
    cap = n // 1000
    for b in range(B):
        px = img[b].permute(1, 2, 0).reshape(-1, 3).numpy()
        wv = None if w is None else w[b].reshape(-1).numpy()
        want, alt = R.quantize(px, wv), R.quantize(px, wv, root='pow')
        # the reference against itself: two fp64 formulations of the chain stay within the cap
        assert np.abs(want - alt).max() <= 1 and int((want != alt).sum()) <= cap
        diff = np.abs(got[b] - want)
        print(f'quantise ({name}, image {b}, {n} pixels): {int((diff > 0).sum())} values differ (cap {cap}), max |q - q_ref| = {diff.max()}')
        assert diff.max() <= 1 and int((diff[:, :3] > 0).sum()) <= cap
        assert np.array_equal(got[b][:, 3], want[:, 3])                                      # weights are exact
        bad = ~(np.isfinite(px).all(axis=1) & (np.ones(n, bool) if wv is None else np.isfinite(wv)))
        assert not got[b][bad].any() and (name != 'small' or bad.sum() == 4)
        if wv is not None:
            assert np.all(got[b][np.nan_to_num(wv, nan=0.0) <= 0, 3] == 0) and (name != 'small' or got[b][:, 3].max() == 65535)


# ---- bins --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SIZE_NAMES)
def test_bins_equal_the_reference(P, SHARE, name):
    n = sizes(SHARE)[name]
    assert P.lib.hg_palette_blocks(n) == {'one': 1, 'share-1': 1, 'share': 1, 'share+1': 2, 'three_workgroups': 3}[name]
    batches = [random_points(n, 20), random_points(n, 21)]
    pts_t = dev_points(P, batches)
    got = gpu_bins(P, pts_t, 2, n).cpu().numpy()
    for b in range(2):
        assert np.array_equal(got[b], R.bins(batches[b]))
    for blocks in (1, 5):                                                                    # a forced count: the same integers
        assert np.array_equal(gpu_bins(P, pts_t, 2, n, blocks).cpu().numpy(), got)
    one = gpu_bins(P, pts_t[1:], 1, n).cpu().numpy()                                         # B = 1 on the second image
    assert np.array_equal(one[0], got[1])


# ---- seeds -------------------------------------------------------------------------------------------------------------------
def crafted_cells(kind):
    cells = np.zeros((R.CELLS, 4), dtype=np.int64)
    rs = np.random.RandomState(31)
    if kind == 'random':
        idx = rs.choice(R.CELLS, 300, replace=False)
        w = rs.randint(1, 2 ** 30, 300).astype(np.int64)
        cells[idx, 0] = w
        cells[idx, 1] = w * rs.randint(0, 12800, 300)
        cells[idx, 2:] = w[:, None] * rs.randint(-12000, 12000, (300, 2))
    elif kind == 'wide':                  # W near 2^43 and d^2 near 2^30: the scores need more than 64 bits, and differ in the low word
        idx = np.array([5, 900, 901, 2000, 4095])
        w = np.array([2 ** 43 + 7, 2 ** 43, 2 ** 43 + 1, 2 ** 43 - 3, 2 ** 43])
        m = np.array([[0, 0, 0], [12000, 16000, 0], [12000, 16000, 0], [12000, -16000, 3], [6000, 0, 16000]])
        cells[idx, 0] = w
        cells[idx, 1:] = w[:, None] * m
    elif kind == 'tie':                   # equal weights everywhere and a symmetric layout: the lowest cell index wins every tie
        idx = np.array([10, 20, 30, 40])
        cells[idx, 0] = 1000
        cells[idx, 1:] = 1000 * np.array([[100, 0, 0], [100, 500, 0], [100, -500, 0], [100, 0, 500]])
    elif kind == 'one_cell':              # all weight in one cell: the seeds duplicate; negative half-way means round up
        cells[77] = (2, 5, -5, -3)
    return cells


@pytest.mark.parametrize('kind', ['random', 'wide', 'tie', 'one_cell', 'empty'])
def test_seeds_equal_the_reference(P, kind):
    cells = crafted_cells(kind)
    if kind == 'wide':
        assert int(cells[:, 0].max()) * (12000 ** 2 + 32000 ** 2) > 2 ** 64
    bins_t = torch.from_numpy(np.stack([cells, crafted_cells('random')])).to(DEV)
    for K in (1, 2, 16):
        got = gpu_seeds(P, bins_t, 2, K).cpu().numpy()
        assert np.array_equal(got[0], R.seeds(cells, K)) and np.array_equal(got[1], R.seeds(crafted_cells('random'), K))
    s = gpu_seeds(P, bins_t, 2, 4).cpu().numpy()[0]
    if kind == 'one_cell':
        assert s.tolist() == [[3, -2, -1]] * 4                     # floor((2 S + W) / (2 W)) of (5, -5, -3) / 2: halves go up
    if kind == 'empty':
        assert not s.any()
    if kind == 'tie':
        assert s[0].tolist() == [100, 0, 0] and s[1].tolist() == [100, 500, 0]


# ---- step and update ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SIZE_NAMES)
def test_step_equals_the_reference(P, SHARE, name):
    n = sizes(SHARE)[name]
    a = [random_points(n, 40), random_points(n, 41)]
    v = [random_points(n, 42), random_points(n, 43)]
    a_t, v_t = dev_points(P, a), dev_points(P, v)
    rs = np.random.RandomState(44)
    for K in (1, 2, 16):
        cen = np.stack([rs.randint(0, 12800, (2, K)), rs.randint(-12000, 12000, (2, K)), rs.randint(-12000, 12000, (2, K))], axis=-1)
        if K == 16:
            cen[0, 9] = cen[0, 4]                                   # a duplicate centre: the lower index takes its points
        start = torch.from_numpy(rs.randint(-1000, 1000, (2, K, 4)).astype(np.int64)).to(DEV)
        for value, val_t in ((a, a_t), (v, v_t)):                   # k-means, and the paired sums
            sums, lab = gpu_step(P, a_t, val_t, 2, n, cen, K, start=start)
            for b in range(2):
                ws, wl = R.step(a[b], value[b], cen[b])
                assert np.array_equal(sums[b].cpu().numpy(), ws + start[b].cpu().numpy())    # added to what was there
                assert np.array_equal(lab[b].cpu().numpy(), wl)
                assert (wl == R.NO_LABEL).sum() == (a[b][:, 3] == 0).sum() and (n < 100 or (wl == R.NO_LABEL).any())
            forced, lab1 = gpu_step(P, a_t, val_t, 2, n, cen, K, blocks=1, start=start)
            assert torch.equal(forced, sums) and torch.equal(lab1, lab)
            nolab, _ = gpu_step(P, a_t, val_t, 2, n, cen, K, blocks=7, start=start, labels=False)
            assert torch.equal(nolab, sums)
        if K == 16:
            assert not (R.step(a[0], a[0], cen[0])[1] == 9).any()


def test_step_ties_take_the_lowest_index(P):
    tp, tc = R.ties()
    t = dev_points(P, [tp])
    sums, lab = gpu_step(P, t, t, 1, len(tp), tc[None], 3)
    ws, wl = R.step(tp, tp, tc)
    d = R.distances(tp, tc)
    assert (d[:, 0] == d[:, 1]).sum() >= len(tp) // 2
    assert np.array_equal(lab[0].cpu().numpy(), wl) and np.array_equal(sums[0].cpu().numpy(), ws)
    assert np.all(lab[0].cpu().numpy()[d[:, 0] == d[:, 1]] == 0)


def test_update_rounds_halves_up_and_keeps_empty_clusters(P):
    sums = np.array([[[2, 5, -5, -3], [0, 99, 99, 99], [3, -4, 4, 0], [2 ** 40, -(2 ** 40) * 9001 - 2 ** 39, 2 ** 53, 7]],
                     [[1, 12800, -16384, 16383], [7, -7, 0, 7], [0, 0, 0, 0], [4, 2, -2, 6]]], dtype=np.int64)
    cen = np.arange(2 * 4 * 3, dtype=np.int32).reshape(2, 4, 3) - 5
    want = np.stack([R.update(sums[b], cen[b]) for b in range(2)])
    assert want[0, 0].tolist() == [3, -2, -1] and want[0, 1].tolist() == cen[0, 1].tolist() and want[0, 3, 0] == -9001
    for clear in (False, True):
        s_t, c_t = torch.from_numpy(sums).to(DEV), torch.from_numpy(cen).to(DEV)
        gpu_update(P, s_t, c_t, clear)
        assert np.array_equal(c_t.cpu().numpy(), want)
        assert (int(s_t.abs().sum()) == 0) if clear else np.array_equal(s_t.cpu().numpy(), sums)


# ---- run ---------------------------------------------------------------------------------------------------------------------
def run_images():
    """(image (2, 3, 96, 100), other, weight (2, 96, 100)): 9600 pixels, three workgroups; smooth, textured, in gamut."""
    rs = np.random.RandomState(50)
    yy, xx = np.mgrid[0:96, 0:100] / 100.0
    a = np.stack([0.5 + 0.4 * np.sin(6 * yy) * np.cos(5 * xx), 0.5 + 0.45 * np.cos(4 * xx + 1), 0.3 + 0.6 * yy * xx]) + rs.normal(0, 0.03, (3, 96, 100))
    b = np.stack([0.2 + 0.7 * (yy > 0.5), 0.5 + 0.3 * np.sin(9 * xx), 0.8 - 0.6 * xx]) + rs.normal(0, 0.02, (3, 96, 100))
    img = np.clip(np.stack([a, b]), 0, 1).astype(np.float32)
    other = np.clip(img[:, [2, 0, 1]] * 0.8 + 0.1, 0, 1).astype(np.float32)
    w = rs.rand(2, 96, 100).astype(np.float32)
    w[:, :10] = 0.0
    return img, other, w


def compose_by_hand(P, x, w, other, K, iterations):
    """hg_palette_run's launch sequence from the stage entry points."""
    lib, st = P.lib, stream(P)
    B, _, H, W = x.shape
    n = H * W
    stride = lib.hg_palette_point_stride(n)
    pts = torch.empty((B, stride, 4), dtype=torch.int16, device=DEV)
    P.check(lib.hg_palette_quantize(x.data_ptr(), *x.stride(), P.ptr(w), *((0, 0, 0) if w is None else w.stride()), pts.data_ptr(),
                                    B, H, W, st), 'hg_palette_quantize')
    centres = gpu_seeds(P, gpu_bins(P, pts, B, n), B, K)
    sums = torch.zeros((B, K, 4), dtype=torch.int64, device=DEV)
    for _ in range(iterations):
        sums, _ = gpu_step(P, pts, pts, B, n, centres, K, start=sums, labels=False)
        gpu_update(P, sums, centres, True)
    sums, labels = gpu_step(P, pts, pts, B, n, centres, K, start=sums)
    centres_other = None
    if other is not None:
        pts2 = torch.empty_like(pts)
        P.check(lib.hg_palette_quantize(other.data_ptr(), *other.stride(), None, 0, 0, 0, pts2.data_ptr(), B, H, W, st),
                'hg_palette_quantize')
        centres_other = centres.clone()
        s2, _ = gpu_step(P, pts, pts2, B, n, centres, K, labels=False)
        gpu_update(P, s2, centres_other, False)
        gpu_update(P, sums, centres, False)
    return centres, sums, centres_other, labels.reshape(B, H, W), pts


@pytest.mark.parametrize('K,iterations,paired', [(8, 6, True), (16, 3, False), (1, 0, True)])
def test_run_equals_the_stages_a_second_run_and_the_reference_bit_for_bit(P, SHARE, K, iterations, paired):
    img, other, w = run_images()
    B, n = 2, 96 * 100
    assert P.lib.hg_palette_blocks(n) == 3
    x, o, wd = torch.from_numpy(img).to(DEV), (torch.from_numpy(other).to(DEV) if paired else None), torch.from_numpy(w).to(DEV)
    first = P._palette_run(x, wd, o, K, iterations, want_labels=True)
    second = P._palette_run(x, wd, o, K, iterations, want_labels=True)
    forced = P._palette_run(x, wd, o, K, iterations, want_labels=True, blocks=1)              # one workgroup per image
    hand = compose_by_hand(P, x, wd, o, K, iterations)
    for other_run in (second, forced, hand[:4]):
        for a, b in zip(first, other_run):
            assert (a is None and b is None) or torch.equal(a, b)
    pts = host_points(hand[4], n)
    pts_o = host_points(compose_by_hand(P, o, None, None, 1, 0)[4], n) if paired else None
    for b in range(B):
        c, sums, labels, co = R.run(pts[b], K, iterations, value=None if pts_o is None else pts_o[b])
        assert np.array_equal(first[0][b].cpu().numpy(), c) and np.array_equal(first[1][b].cpu().numpy(), sums)
        assert np.array_equal(first[3][b].cpu().numpy().reshape(-1), labels)
        assert co is None or np.array_equal(first[2][b].cpu().numpy(), co)
        assert int(sums[:, 0].sum()) == int(pts[b][:, 3].sum()) and (labels[:1000] == R.NO_LABEL).all()     # the weightless rows
    assert np.array_equal(x.cpu().numpy(), img)                                                # the inputs are only read


# ---- the Python surface of the extraction ----------------------------------------------------------------------------------
def test_palette_paired_palette_and_labels(P):
    img, other, w = run_images()
    x, o, wd = torch.from_numpy(img).to(DEV), torch.from_numpy(other).to(DEV), torch.from_numpy(w).to(DEV)
    K = 5
    pal = P.palette(x, k=K, iterations=4, weight=wd)
    assert isinstance(pal, P.Palette) and pal.rgb.shape == (2, K, 3) and pal.lab.shape == (2, K, 3) and pal.weight.shape == (2, K)
    centres, sums, _, _ = P._palette_run(x, wd, None, K, 4)
    W = sums[..., 0].cpu().numpy()
    for b in range(2):
        order = np.argsort(-W[b], kind='stable')
        assert np.array_equal(pal.lab[b].cpu().numpy(), centres[b].cpu().numpy()[order] / np.float32(R.UNIT))
        assert np.allclose(pal.weight[b].cpu().numpy(), W[b][order] / W[b].sum(), rtol=1e-6, atol=0)
        assert np.all(np.diff(pal.weight[b].cpu().numpy()) <= 0) and abs(float(pal.weight[b].sum()) - 1) <= 1e-6
        assert np.abs(pal.rgb[b].cpu().numpy() - R.lab_to_srgb(pal.lab[b].cpu().numpy().astype(np.float64))).max() <= 2e-6
    raw = P.palette(x, k=K, iterations=4, weight=wd, sort=False)
    assert np.array_equal(raw.lab.cpu().numpy(), centres.cpu().numpy() / np.float32(R.UNIT))
    # one image: the same palette without the batch axis; (H, W) weight
    one = P.palette(x[1], k=K, iterations=4, weight=wd[1])
    assert one.lab.shape == (K, 3) and torch.equal(one.lab, pal.lab[1]) and torch.equal(one.weight, pal.weight[1])
    # fewer colours than K: the empty clusters trail with weight 0
    flat = torch.zeros(3, 8, 8, device=DEV)
    flat[:, :, 4:] = 1.0
    few = P.palette(flat, k=4, iterations=2)
    assert few.weight.cpu().tolist() == [0.5, 0.5, 0.0, 0.0] and np.abs(few.rgb[:2].cpu().numpy().sum(axis=1) - [0, 3]).max() <= 1e-5
    # labels against given centres, as the reference assigns the same points
    lab = P.palette_labels(x, raw).cpu().numpy()
    pts = host_points(compose_by_hand(P, x, None, None, 1, 0)[4], 9600)
    for b in range(2):
        assert np.array_equal(lab[b].reshape(-1), R.step(pts[b], pts[b], centres[b].cpu().numpy())[1])
    assert torch.equal(P.palette_labels(x[0], P.Palette(raw.rgb[0], raw.lab[0], raw.weight[0])), torch.from_numpy(lab[0]).to(DEV))
    # the paired palette: both are means over the clusters of the last step; an image with itself gives dst == src
    src, dst = P.paired_palette(x[0], o[0], k=K, iterations=4, weight=wd[0])
    c, sums, co, _ = P._palette_run(x[:1], wd[:1], o[:1], K, 4)
    order = np.argsort(-sums[0, :, 0].cpu().numpy(), kind='stable')
    assert np.array_equal(src.lab.cpu().numpy(), c[0].cpu().numpy()[order] / np.float32(R.UNIT))
    assert np.array_equal(dst.lab.cpu().numpy(), co[0].cpu().numpy()[order] / np.float32(R.UNIT)) and torch.equal(src.weight, dst.weight)
    same_s, same_d = P.paired_palette(x[0], x[0], k=K, iterations=1)
    assert torch.equal(same_s.lab, same_d.lab) and torch.equal(same_s.rgb, same_d.rgb)
    e_s, e_d = P.paired_palette(flat, 1 - flat, k=3, iterations=2)
    assert float(e_s.weight[2]) == 0.0 and torch.equal(e_s.lab[2], e_d.lab[2]) and not torch.equal(e_s.lab[0], e_d.lab[0])


def test_match_palettes_pairs_by_rank_of_lightness(P):
    mk = lambda L: P.Palette(torch.rand(len(L), 3, device=DEV), torch.tensor([[v, i, -i] for i, v in enumerate(L)], device=DEV),    # noqa: E731
                             torch.arange(len(L), device=DEV) / 10.0)
    src, dst = mk([50.0, 10.0, 90.0, 30.0]), mk([5.0, 80.0, 40.0, 60.0])
    out = P.match_palettes(src, dst)
    assert out.lab[:, 0].cpu().tolist() == [60.0, 5.0, 80.0, 40.0]                     # ranks 2, 0, 3, 1 of dst's lightness
    assert out.weight.cpu().tolist() == pytest.approx([0.3, 0.0, 0.1, 0.2]) and torch.equal(out.rgb[1], dst.rgb[0])
    typed = P.palette_from_rgb(torch.tensor([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], device=DEV))
    assert np.abs(typed.lab.cpu().numpy() - R.srgb_to_lab(typed.rgb.cpu().numpy())).max() <= 1e-4 and float(typed.weight.sum()) == pytest.approx(1)


# ---- transfer ----------------------------------------------------------------------------------------------------------------
PHOTO_HW = R.PHOTO_HW
_REFERENCE = {}


def reference(name):
    """(fp64 result, eps32, sigma) of one case of palette_ref.transfer_case; computed once, shared, never modified."""
    if name not in _REFERENCE:
        px, src, dst, live, sigma = R.transfer_case(name)
        a, sg = R.transfer(px, src, dst, live, sigma)
        b, _ = R.transfer(px, src, dst, live, sigma, dtype=np.float32)
        a.setflags(write=False)
        _REFERENCE[name] = (a, float(np.abs(a - b).max()), sg)
    return _REFERENCE[name]


def palettes_on_device(P, src, dst, live):
    wt = torch.from_numpy(np.where(live, 1.0 / len(src), 0.0).astype(np.float32)).to(DEV)
    mk = lambda lab: P.Palette(torch.zeros(len(lab), 3, device=DEV), torch.from_numpy(lab).to(DEV), wt)       # noqa: E731
    return mk(src), mk(dst)


@pytest.mark.parametrize('name', R.TRANSFER_CASES + ('strided',))
def test_transfer_against_fp64(P, name):
    case = 'default_sigma' if name == 'strided' else name
    px, src, dst, live, sigma = R.transfer_case(case)
    want, eps32, sg = reference(case)
    ps, pd = palettes_on_device(P, src, dst, live)
    x = torch.from_numpy(px).to(DEV)
    if name == 'strided':                                    # a CHW image's permuted view: no copy is made
        x = x.permute(2, 0, 1).contiguous().permute(1, 2, 0)
        assert not x.is_contiguous() and x.stride(2) == PHOTO_HW[0] * PHOTO_HW[1]
    out, used = P.color_transfer_palette(x, ps, pd, sigma=sigma)
    assert out.shape == px.shape and out.dtype == torch.float32 and used.shape == () and used.device == out.device
    assert float(used) == pytest.approx(sg, rel=1e-6) and (case != 'one_colour' or float(used) == 1.0)
    err = float(np.abs(out.cpu().numpy() - want).max())
    print(f'transfer ({name}, sigma {float(used):.2f}): eps32 {eps32:.2e}, kernel error {err:.2e}, bar {4 * eps32:.2e}')
    assert eps32 <= 1e-5, 'ill-conditioned input: the fp32 and fp64 references disagree by more than 1e-5'
    assert err <= 4 * eps32
    if name == 'identity':
        assert float(np.abs(out.cpu().numpy() - px).max()) <= 4 * eps32
    if name == 'not_live':                                   # the dead cluster pulls nothing, whatever its destination says
        pd2 = P.Palette(pd.rgb, pd.lab + torch.tensor([[0.0], [0.0], [40.0], [0.0], [0.0], [0.0]], device=DEV), pd.weight)
        assert torch.equal(P.color_transfer_palette(x, ps, pd2)[0], out)
    # the quantised output: one 8-bit level, on at most 0.1 % of the values
    q, _ = P.color_transfer_palette(x, ps, pd, sigma=sigma, quantize=True)
    assert q.dtype == torch.uint8 and torch.equal(q, (out * 255.0).to(torch.uint8))
    dq = np.abs(q.cpu().numpy().astype(int) - R.to_u8(want).astype(int))
    print(f'    quantised: {int((dq > 0).sum())} of {dq.size} values differ from the reference')
    assert dq.max() <= 1 and int((dq > 0).sum()) <= dq.size // 1000
    assert torch.equal(P.color_transfer_palette(x, ps, pd, sigma=sigma)[0], out)             # repeats are bit-identical


def test_transfer_follows_per_blob_shifts_better_than_the_affine_map(P):
    K = 6
    px, blob = R.clustered(K=K, per_blob=150, seed=2)
    tgt = R.shifted(px, blob, K, seed=2)
    img, oth = (torch.from_numpy(a.T.reshape(3, 30, 30).copy()).to(DEV) for a in (px, tgt))
    src, dst = P.paired_palette(img, oth, k=K, iterations=8)
    assert float(src.weight.min()) > 0
    sigma = R.separating_sigma(src.lab.cpu().numpy())
    hwc = img.permute(1, 2, 0)
    pal, _ = P.color_transfer_palette(hwc, src, dst, sigma=sigma)
    mkl, _ = P.color_transfer_mkl(hwc, oth.permute(1, 2, 0))
    want = tgt.reshape(30, 30, 3)
    e_pal, e_mkl = float(np.abs(pal.cpu().numpy() - want).mean()), float(np.abs(mkl.cpu().numpy() - want).mean())
    print(f'per-blob shifts, mean |out - shifted|: palette transfer {e_pal:.2e} (sigma {sigma:.2f}), MKL {e_mkl:.2e}')
    assert e_pal < e_mkl


# ---- palette_histogram -------------------------------------------------------------------------------------------------------
def test_palette_histogram_drives_the_histogram_blocks(P):
    from histogram_classes.LabHistBlock import LabHistBlock
    from histogram_classes.RGBuvHistBlock import RGBuvHistBlock
    from histogram_classes.rgChromaHistBlock import rgChromaHistBlock
    x = torch.from_numpy(R.smooth(32, 32).transpose(2, 0, 1).copy()).to(DEV)
    pal = P.palette(x, k=5, iterations=4)
    img, wt = pal.rgb.t().reshape(1, 3, 1, 5).contiguous(), pal.weight.reshape(1, 1, 5)
    for block in (RGBuvHistBlock(h=16, device=DEV), rgChromaHistBlock(h=16, device=DEV), LabHistBlock(h=16, device=DEV, from_rgb=True)):
        h = P.palette_histogram(block, pal)
        # the blocks divide by the raw mass S + 1e-6 (include/hg_hist.h), so the sum is S / (S + 1e-6): within 1e-3 of 1 for any
        # S >= 1e-3, which K colours of total weight 1 have unless all of them are black
        assert torch.equal(h, block(img, weight=wt)) and abs(float(h.sum()) - 1.0) <= 1e-3 and float(h.min()) >= 0
    lab_block = LabHistBlock(h=16, device=DEV)
    assert torch.allclose(P.palette_histogram(lab_block, pal), lab_block(P.srgb_to_lab(img), weight=wt), atol=1e-4)
    batch = P.palette(torch.stack([x, x.flip(0)]), k=5, iterations=4)
    hb = P.palette_histogram(RGBuvHistBlock(h=16, device=DEV), batch)
    assert hb.shape == (2, 3, 16, 16) and torch.allclose(hb.sum(dim=(1, 2, 3)), torch.ones(2, device=DEV), atol=1e-3)


# ---- recoloringTrainer.evaluate --------------------------------------------------------------------------------------------
def test_evaluate_post_recoloring_palette(P, tmp_path, monkeypatch):
    torch.manual_seed(0)
    from ReHistoGAN.rehistoGAN import recoloringTrainer
    from histogram_classes.RGBuvHistBlock import RGBuvHistBlock
    tr = recoloringTrainer('palette', str(tmp_path / 'results'), str(tmp_path / 'models'), image_size=64, network_capacity=4,
                           batch_size=1, hist_bin=16, hist_insz=32)
    tr.init_GAN()
    photo = R.smooth(40, 52).astype(np.float64)                     # (H, W, 3) in [0, 1], as evaluate receives it
    img = torch.rand(1, 3, 64, 64, device=DEV)
    # the target histogram comes from five colours: a valid hist_batch
    five = P.palette_from_rgb(torch.tensor([[0.9, 0.2, 0.1], [0.1, 0.3, 0.8], [0.9, 0.8, 0.2], [0.1, 0.1, 0.1], [0.6, 0.9, 0.6]], device=DEV))
    h = P.palette_histogram(RGBuvHistBlock(h=16, device=DEV), five)
    assert h.shape == (1, 3, 16, 16)
    writes = []
    real = P.save_rgb
    monkeypatch.setattr(P, 'save_rgb', lambda a, p: (writes.append(a.clone()), real(a, p)))
    src = torch.from_numpy(np.ascontiguousarray(photo, dtype=np.float32)).to(DEV)
    outs = {}
    for mode in ('palette', True):
        with torch.no_grad():
            g = tr.evaluate(f'out_{mode}', image_batch=img, hist_batch=h, original_image=photo, save_input=False,
                            post_recoloring=mode)
        assert len(writes) == 1 and writes[0].dtype == torch.uint8 and writes[0].shape == (40, 52, 3)
        if mode == 'palette':
            ps, pd = P.paired_palette(img[0], g[0], k=8)
            assert torch.equal(writes[0], P.color_transfer_palette(src, ps, pd, quantize=True)[0])
        else:
            assert torch.equal(writes[0], P.color_transfer_mkl(src, g[0].permute(1, 2, 0), quantize=True)[0])
        outs[mode] = (writes.pop(), g)
    g = outs['palette'][1]
    assert not torch.equal(outs['palette'][0], P.color_transfer_mkl(src, g[0].permute(1, 2, 0), quantize=True)[0])
    with pytest.raises(ValueError, match='post_recoloring'):
        tr.evaluate('bad', image_batch=img, hist_batch=h, original_image=photo, post_recoloring='nonsense')
