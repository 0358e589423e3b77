"""The iterative distribution transfer on the GPU (hg_idt_*, include/hg_post.h; post.color_transfer_idt;
recoloringTrainer.evaluate(post_recoloring='idt')) against the fp64 restatement tests/idt_ref.py.

Stage bars (each stage gets its inputs handed in, so nothing upstream blurs them):
  range      abs <= 2^-21: an fp32 projection of inputs in [0, 1] is three products and two sums of magnitude <= sqrt(3)
  histogram  sum_k h[k] == 65536 N exactly; sum_k |h - h_ref| <= 2 N (65536 du + 1), du = 2^-21 (n - 1) / (hi - lo): the
             projection bar carried into node units, plus the rounding of q
  table      relmax <= 2^-23: the integers are exact on both sides, only the fp64 division and the fp32 store round
  apply      abs <= (1 + L) 2^-20, L the largest slope |M[k+1] - M[k]| (n - 1) / (hi0 - lo0) of the handed-in maps
End to end the bar is 4 eps32, eps32 being the largest difference between the reference run in fp64 and in fp32 arithmetic
on the same inputs (the operator's own noise floor at the kernels' precision); a case whose eps32 exceeds 1e-5 is an
ill-conditioned input and fails as such.  Measured on the MI355X (10 rotations, 1280-pixel source, 1024-pixel target):

    target   bins   eps32     kernel error
    smooth    16    4.29e-07  4.48e-07
    smooth    32    5.44e-07  6.16e-07
    smooth    64    1.12e-06  1.29e-06
    bimodal   16    3.95e-06  3.95e-06
    bimodal   32    2.97e-06  3.50e-06
    bimodal   64    7.07e-06  3.35e-06

Self-transfer moves pixels by at most 2^-20; hg_idt_run, the stages composed by hand and a second run give the same bits."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import idt_ref as R
from conftest import relmax

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)


@pytest.fixture(scope='module')
def P():
    from histogan_amd import build
    build.build()
    from histogan_amd import post
    return post


@pytest.fixture(scope='module')
def K(P):
    """The exported constants every shape below is derived from."""
    lib = P.lib
    k = dict(block_pixels=lib.hg_idt_block_pixels(), group=lib.hg_idt_group_pixels(), max_bins=lib.hg_idt_max_bins())
    n = 1
    while lib.hg_idt_blocks(n + 1) == 1:          # the largest count one workgroup takes (doubling, then bisecting)
        n *= 2
    lo, hi = n // 2, n + 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lib.hg_idt_blocks(mid) == 1 else (lo, mid)
    k['share'] = lo
    return k


# ---- plumbing: the stage entry points on torch tensors -----------------------------------------------------------------
def stream(P):
    return P.raw_stream(DEV)


def dev_rot(rots):
    return torch.from_numpy(np.ascontiguousarray(rots, dtype=np.float32).reshape(-1, 3, 3)).to(DEV)


def pixels(n, seed, lo=0.0, hi=1.0):
    return np.random.RandomState(seed).uniform(lo, hi, (n, 3)).astype(np.float32)


def make_planes(P, x):
    """(planes tensor (3, stride), stride) of (N, 3) pixels; the padding holds NaN: it must never reach a result."""
    n = x.shape[0]
    st = P.lib.hg_idt_plane_stride(n)
    pl = np.full((3, st), np.nan, dtype=np.float32)
    pl[:, :n] = x.T
    return torch.from_numpy(pl).to(DEV), st


def cleared(P, n_sets, n_counters):
    rng = torch.empty(max(n_sets, 1) * 6, dtype=torch.int32, device=DEV)
    hist = torch.empty(max(n_counters, 1), dtype=torch.int64, device=DEV)
    P.check(P.lib.hg_idt_clear(rng.data_ptr(), n_sets, hist.data_ptr(), n_counters, stream(P)), 'hg_idt_clear')
    return rng, hist


def gpu_ranges(P, x_t, n, ps, cs, rots, planes=None):
    rng, _ = cleared(P, len(rots), 0)
    rot = dev_rot(rots)
    P.check(P.lib.hg_idt_range(x_t.data_ptr(), n, ps, cs, rot.data_ptr(), len(rots), rng.data_ptr(),
                               None if planes is None else planes.data_ptr(), stream(P)), 'hg_idt_range')
    lo, hi = P.idt_decode_range(rng.cpu().numpy().reshape(len(rots), 6))
    return rng, lo.astype(np.float64), hi.astype(np.float64)


def gpu_hist(P, x_t, n, ps, cs, rots, bins, rng_t, blocks=0):
    _, hist = cleared(P, 0, len(rots) * 3 * bins)
    rot = dev_rot(rots)
    P.check(P.lib.hg_idt_hist(x_t.data_ptr(), n, ps, cs, rot.data_ptr(), len(rots), bins, rng_t.data_ptr(), hist.data_ptr(),
                              blocks, stream(P)), 'hg_idt_hist')
    return hist


def ref_ranges32(x, rots):
    """Per rotation the fp64 min / max of the projections, rounded to the fp32 the kernels are handed."""
    out = [R.ranges(R.project(x, Rm)) for Rm in rots]
    return (np.stack([o[0] for o in out]).astype(np.float32), np.stack([o[1] for o in out]).astype(np.float32))


def range_sets(P, lo, hi):
    enc = np.stack([P.idt_encode_range(lo[i], hi[i]) for i in range(len(lo))])
    return P.idt_range_tensor(enc.reshape(-1), DEV)


def hist_bound(n_pix, bins, lo, hi):
    return 2 * n_pix * (R.UNITS * 2.0 ** -21 * (bins - 1) / (float(hi) - float(lo)) + 1)


def pixel_counts(K):
    """name -> pixel count, each with the structure it is there for (asserted where it is used)."""
    return {'one_row': 37, 'ragged': K['group'] + 17, 'two_workgroups': K['share'] + 5, 'three_workgroups': 2 * K['share'] + 1026}


# ---- range ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['one_row', 'ragged', 'two_workgroups', 'three_workgroups'])
def test_range_against_fp64(P, K, name):
    n = pixel_counts(K)[name]
    blocks = P.lib.hg_idt_blocks(n)
    assert {'one_row': n < 64, 'ragged': n % K['group'] != 0 and n > K['group'] and blocks == 1, 'two_workgroups': blocks == 2,
            'three_workgroups': blocks == 3}[name]
    x = pixels(n, 1)
    rots = R.rotations(4, seed=5)
    xt = torch.from_numpy(x).to(DEV)
    st = P.lib.hg_idt_plane_stride(n)
    planes = torch.full((3, st), float('nan'), device=DEV)
    _, lo, hi = gpu_ranges(P, xt, n, 3, 1, rots, planes)
    want = [R.ranges(R.project(x, Rm)) for Rm in rots]
    err = max(np.abs(lo - np.stack([w[0] for w in want])).max(), np.abs(hi - np.stack([w[1] for w in want])).max())
    print(f'range ({name}, {n} pixels, {blocks} workgroups): abs err {err:.2e} (bar {2.0 ** -21:.2e})')
    assert err <= 2.0 ** -21
    assert np.array_equal(lo[0], x.min(0)) and np.array_equal(hi[0], x.max(0))            # R_0 = I projects exactly
    assert torch.equal(planes[:, :n], xt.t()) and bool(torch.isnan(planes[:, n:]).all())   # the working copy, padding untouched
    # a permuted CHW view gives the same bits without a copy
    chw = torch.from_numpy(np.ascontiguousarray(x.T)).to(DEV)
    _, lo2, hi2 = gpu_ranges(P, chw, n, 1, n, rots)
    assert np.array_equal(lo, lo2) and np.array_equal(hi, hi2)


# ---- histogram -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,bins', [('one_row', 16), ('ragged', 64), ('two_workgroups', 257), ('three_workgroups', 32),
                                       ('second_pass', 64)])
def test_histogram_against_fp64(P, K, name, bins):
    if name == 'second_pass':
        n, blocks = K['block_pixels'] + 1, 1                 # one workgroup's share exceeds a pass over its LDS counters
        assert n > K['block_pixels'] and K['block_pixels'] * R.UNITS < 2 ** 32 <= (K['block_pixels'] + 4) * R.UNITS
    else:
        n, blocks = pixel_counts(K)[name], 0
    x = pixels(n, 2)
    rots = np.concatenate([np.eye(3)[None], R.rotations(3, seed=6)[1:]])
    lo, hi = ref_ranges32(x, rots)
    rng = range_sets(P, lo, hi)
    planes, st = make_planes(P, x)
    nr = len(rots)
    assert nr <= P.lib.hg_idt_target_chunk(bins)
    h = gpu_hist(P, planes, n, 1, st, rots, bins, rng, blocks).cpu().numpy().reshape(nr, 3, bins)
    for r in range(nr):
        v = R.project(x, rots[r])
        for a in range(3):
            want = R.histogram(v[:, a], lo[r, a], hi[r, a], bins)
            dev, bar = int(np.abs(h[r, a] - want).sum()), hist_bound(n, bins, lo[r, a], hi[r, a])
            if a == 0:
                print(f'histogram ({name}, {n} px, {bins} nodes, rotation {r}): sum |h - h_ref| = {dev} (bar {bar:.0f}, '
                      f'{dev / (R.UNITS * n):.2e} of the mass)')
            assert int(h[r, a].sum()) == R.UNITS * n and h[r, a].min() >= 0
            assert dev <= bar
    # the strided (HWC) read and one rotation per launch give the same integers
    xt = torch.from_numpy(x).to(DEV)
    assert np.array_equal(gpu_hist(P, xt, n, 3, 1, rots, bins, rng, blocks).cpu().numpy().reshape(nr, 3, bins), h)
    one = gpu_hist(P, planes, n, 1, st, rots[1:2], bins, rng[6:12], blocks).cpu().numpy().reshape(3, bins)
    assert np.array_equal(one, h[1])


def test_target_tables_second_chunk(P, K):
    """iterations = hg_idt_target_chunk(bins) + 1: the last rotation's counters come from a second histogram launch."""
    bins = 1024
    chunk = P.lib.hg_idt_target_chunk(bins)
    iters = chunk + 1
    assert 1 <= chunk <= 8
    n = 1500
    y = pixels(n, 3, 0.1, 0.9)
    rots = R.rotations(iters, seed=7)
    yt = torch.from_numpy(y).to(DEV)
    rng = torch.zeros(iters * 6, dtype=torch.int32, device=DEV)               # not cleared: the call clears
    hist = torch.full((iters * 3 * bins,), 12345, dtype=torch.int64, device=DEV)
    rot = dev_rot(rots)
    P.check(P.lib.hg_idt_target_tables(yt.data_ptr(), n, 3, 1, rot.data_ptr(), iters, bins, rng.data_ptr(), hist.data_ptr(),
                                       stream(P)), 'hg_idt_target_tables')
    lo, hi = P.idt_decode_range(rng.cpu().numpy().reshape(iters, 6))
    h = hist.cpu().numpy().reshape(iters, 3, bins)
    for r in range(iters):
        v = R.project(y, rots[r])
        wlo, whi = R.ranges(v)
        assert max(np.abs(lo[r] - wlo).max(), np.abs(hi[r] - whi).max()) <= 2.0 ** -21
        one = gpu_hist(P, yt, n, 3, 1, rots[r:r + 1], bins, rng[6 * r:6 * r + 6]).cpu().numpy().reshape(3, bins)
        assert np.array_equal(one, h[r])                                       # chunked == one rotation at a time
        for a in range(3):
            want = R.histogram(v[:, a], lo[r, a], hi[r, a], bins)
            assert int(h[r, a].sum()) == R.UNITS * n
            assert int(np.abs(h[r, a] - want).sum()) <= hist_bound(n, bins, lo[r, a], hi[r, a])


# ---- table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bins,scale', [(2, 1), (16, 1000), (300, 2 ** 20), (4096, 2 ** 36)])
def test_table_against_fp64(P, bins, scale):
    """Integer histograms handed in -- some with totals whose products need more than 64 bits -- with empty stretches."""
    assert bins <= P.lib.hg_idt_max_bins()
    rs = np.random.RandomState(bins)
    h0 = (rs.randint(0, 50, (3, bins)) * (rs.rand(3, bins) < 0.8)).astype(np.int64) * scale
    h1 = (rs.randint(0, 70, (3, bins)) * (rs.rand(3, bins) < 0.7)).astype(np.int64) * (scale // 3 + 1)
    h0[:, -1] += 1
    h1[:, 0] += 2
    h1[:, -1] += 1
    if bins >= 16:
        h1[1, 3:9] = 0                                             # a flat stretch of the target CDF
        h0[2, :] = h1[2, :]                                        # equal histograms: the node grid
    if scale > 2 ** 30:
        assert int(h0[0].sum()) * int(h1[0].sum()) > 2 ** 64
    lo1, hi1 = np.array([-0.7, 0.1, 0.25], dtype=np.float32), np.array([0.9, 1.6, 0.25 + 2.0 ** -10], dtype=np.float32)
    h0_t, h1_t = torch.from_numpy(h0.reshape(-1)).to(DEV), torch.from_numpy(h1.reshape(-1)).to(DEV)
    rng = range_sets(P, lo1[None], hi1[None])
    m = torch.empty(3 * bins, dtype=torch.float32, device=DEV)
    nxt = torch.full((6,), 77, dtype=torch.int32, device=DEV)
    P.check(P.lib.hg_idt_table(h0_t.data_ptr(), h1_t.data_ptr(), rng.data_ptr(), bins, m.data_ptr(), None, 0, stream(P)),
            'hg_idt_table')
    got = m.cpu().numpy().reshape(3, bins)
    assert np.array_equal(h0_t.cpu().numpy().reshape(3, bins), h0) and int(nxt[0]) == 77     # nothing cleared unless asked
    for a in range(3):
        want = R.quantile_map(h0[a], h1[a], lo1[a], hi1[a])
        err = relmax(got[a], want)
        print(f'table ({bins} nodes, counts x {scale}, axis {a}): relmax {err:.2e} (bar {2.0 ** -23:.2e})')
        assert err <= 2.0 ** -23
        assert np.all(np.diff(got[a]) >= 0)                        # a quantile map is monotone
    P.check(P.lib.hg_idt_table(h0_t.data_ptr(), h1_t.data_ptr(), rng.data_ptr(), bins, m.data_ptr(), nxt.data_ptr(), 1,
                               stream(P)), 'hg_idt_table')
    assert np.array_equal(m.cpu().numpy().reshape(3, bins), got)
    assert int(h0_t.abs().sum()) == 0 and np.array_equal(h1_t.cpu().numpy().reshape(3, bins), h1)
    assert np.array_equal(nxt.cpu().numpy().view(np.uint32), np.array([0xffffffff] * 3 + [0] * 3, dtype=np.uint32))


# ---- apply -----------------------------------------------------------------------------------------------------------------
def handed_maps(rs, bins, lo, hi):
    """Monotone maps of three axes onto other ranges, as the kernels hold them (fp32), and the largest slope L of the maps
    of the live axes (hi - lo > 2^-20)."""
    M = np.empty((3, bins), dtype=np.float32)
    L = 0.0
    for a in range(3):
        steps = rs.uniform(0.2, 3.0, bins - 1)
        cdf = np.concatenate([[0.0], np.cumsum(steps)]) / steps.sum()
        width = max(float(hi[a]) - float(lo[a]), 0.5)
        M[a] = (lo[a] - 0.05 + cdf * width * 1.15).astype(np.float32)
        if float(hi[a]) - float(lo[a]) > 2.0 ** -20:
            L = max(L, float(np.abs(np.diff(M[a].astype(np.float64))).max() * (bins - 1) / (float(hi[a]) - float(lo[a]))))
    return M, L


@pytest.mark.parametrize('name,bins,rho', [('one_row', 16, 1.0), ('ragged', 64, 0.7), ('two_workgroups', 33, 1.0),
                                           ('three_workgroups', 256, 0.5)])
def test_apply_against_fp64(P, K, name, bins, rho):
    n = pixel_counts(K)[name]
    x = pixels(n, 4, 0.05, 0.95)
    rs = np.random.RandomState(11)
    Rm, Rn = R.rotations(3, seed=8)[1:]
    lo, hi = ref_ranges32(x, [Rm])
    M, L = handed_maps(rs, bins, lo[0], hi[0])
    rng = range_sets(P, lo, hi)
    m_t = torch.from_numpy(M.reshape(-1)).to(DEV)
    rot, rot_n = dev_rot([Rm]), dev_rot([Rn])
    want = R.apply_maps(x, Rm, lo[0], hi[0], M, bins, rho)
    bar = (1 + L) * 2.0 ** -20
    # a middle rotation: the planes are updated in place and the next rotation's range comes out of the same pass
    planes, st = make_planes(P, x)
    nxt, _ = cleared(P, 1, 0)
    P.check(P.lib.hg_idt_apply(planes.data_ptr(), n, rot.data_ptr(), rot_n.data_ptr(), bins, rng.data_ptr(), m_t.data_ptr(), rho,
                               nxt.data_ptr(), None, 0, stream(P)), 'hg_idt_apply')
    got = planes[:, :n].t().cpu().numpy()
    err = float(np.abs(got - want).max())
    print(f'apply ({name}, {n} px, {bins} nodes, rho {rho}): abs err {err:.2e}, largest slope L = {L:.2f}, bar {bar:.2e}')
    assert err <= bar
    nlo, nhi = P.idt_decode_range(nxt.cpu().numpy().reshape(1, 6))
    wlo, whi = R.ranges(R.project(got, Rn))                       # of the pixels the kernel wrote: the range bar applies
    assert max(np.abs(nlo[0] - wlo).max(), np.abs(nhi[0] - whi).max()) <= 2.0 ** -21
    # the last rotation: clipped, HWC, fp32 and uint8
    planes, st = make_planes(P, x)
    out = torch.full((n, 3), float('nan'), device=DEV)
    P.check(P.lib.hg_idt_apply(planes.data_ptr(), n, rot.data_ptr(), None, bins, rng.data_ptr(), m_t.data_ptr(), rho, None,
                               out.data_ptr(), 0, stream(P)), 'hg_idt_apply')
    assert float(np.abs(out.cpu().numpy() - np.clip(want, 0, 1)).max()) <= bar
    assert torch.equal(out, planes.new_tensor(np.clip(got, 0, 1)))                 # the same arithmetic, then the clip
    assert torch.equal(planes[:, :n].t(), torch.from_numpy(x).to(DEV))             # the last rotation leaves the planes alone
    u8 = torch.full((n, 3), 99, dtype=torch.uint8, device=DEV)
    P.check(P.lib.hg_idt_apply(planes.data_ptr(), n, rot.data_ptr(), None, bins, rng.data_ptr(), m_t.data_ptr(), rho, None,
                               u8.data_ptr(), 1, stream(P)), 'hg_idt_apply')
    assert torch.equal(u8, (out * 255.0).to(torch.uint8))


def test_apply_degenerate_axis_does_not_move(P):
    """A source axis with hi0 - lo0 <= 2^-20 is left alone whatever its map says; the other two move."""
    n, bins = 300, 16
    x = pixels(n, 5, 0.2, 0.8)
    x[:, 1] = 0.5 + np.random.RandomState(1).randint(0, 2, n) * 2.0 ** -21       # below the threshold, not constant
    lo, hi = ref_ranges32(x, [np.eye(3)])
    assert 0 < hi[0, 1] - lo[0, 1] <= 2.0 ** -20
    M, L = handed_maps(np.random.RandomState(2), bins, lo[0], hi[0])
    assert np.abs(M[1] - x[:, 1].mean()).max() > 0.04             # the dead axis' map would move its pixels if it were used
    want = R.apply_maps(x, np.eye(3), lo[0], hi[0], M, bins)
    planes, st = make_planes(P, x)
    out = torch.empty((n, 3), device=DEV)
    rot, rng, m_t = dev_rot([np.eye(3)]), range_sets(P, lo, hi), torch.from_numpy(M.reshape(-1)).to(DEV)
    P.check(P.lib.hg_idt_apply(planes.data_ptr(), n, rot.data_ptr(), None, bins, rng.data_ptr(), m_t.data_ptr(), 1.0, None,
                               out.data_ptr(), 0, stream(P)), 'hg_idt_apply')
    got = out.cpu().numpy()
    assert np.array_equal(got[:, 1], x[:, 1]) and np.abs(got - np.clip(want, 0, 1)).max() <= (1 + L) * 2.0 ** -20
    assert np.abs(got[:, 0] - x[:, 0]).max() > 1e-3


# ---- end to end ------------------------------------------------------------------------------------------------------------
ITERS = 10


@lru_cache(maxsize=None)
def reference(kind, bins):
    """(fp64 result, eps32) of one seeded case; computed once, shared, never modified."""
    s, t = R.seeded_pair(kind)
    rots = R.rotations(ITERS)
    a = R.transfer(s, t, rots, bins)
    b = R.transfer(s, t, rots, bins, dtype=np.float32)
    a.setflags(write=False)
    return a, float(np.abs(a - b).max())


@pytest.mark.parametrize('bins', [16, 32, 64])
@pytest.mark.parametrize('kind', ['smooth', 'bimodal'])
def test_transfer_against_fp64(P, kind, bins):
    s, t = R.seeded_pair(kind)
    assert s.shape[:2] != t.shape[:2] and bins * 16 <= min(s.shape[0] * s.shape[1], t.shape[0] * t.shape[1])
    want, eps32 = reference(kind, bins)
    out, rots = P.color_transfer_idt(torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV), iterations=ITERS, bins=bins)
    assert np.array_equal(rots, R.rotations(ITERS)) and out.shape == s.shape and out.dtype == torch.float32
    err = float(np.abs(out.cpu().numpy() - want).max())
    print(f'transfer ({kind}, {bins} bins, {ITERS} rotations): eps32 {eps32:.2e}, kernel error {err:.2e}, bar {4 * eps32:.2e}')
    assert eps32 <= 1e-5, 'ill-conditioned input: the fp32 and fp64 references disagree by more than 1e-5'
    assert err <= 4 * eps32


def test_transfer_of_a_permuted_chw_view_and_one_pixel_row(P):
    s, t = R.seeded_pair('smooth')
    sd, td = torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV)
    base, _ = P.color_transfer_idt(sd, td, iterations=4, bins=32)
    chw_s, chw_t = sd.permute(2, 0, 1).contiguous(), td.permute(2, 0, 1).contiguous()
    view = chw_s.permute(1, 2, 0)
    assert not view.is_contiguous() and view.stride(2) == s.shape[0] * s.shape[1]
    out, _ = P.color_transfer_idt(view, chw_t.permute(1, 2, 0), iterations=4, bins=32)
    assert torch.equal(out, base)                                  # the strides are honoured on the first read only
    # the same pixels as one row: the transfer does not see the image's shape
    row, _ = P.color_transfer_idt(sd.reshape(1, -1, 3), td.reshape(1, -1, 3), iterations=4, bins=32)
    assert row.shape == (1, s.shape[0] * s.shape[1], 3) and torch.equal(row.reshape(base.shape), base)


def test_constant_source_and_constant_target(P):
    s, t = R.seeded_pair('bimodal')
    sd, td = torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV)
    # a constant source: every axis of every rotation is degenerate, nothing moves, nothing divides by zero
    const = torch.empty_like(sd)
    const[:] = torch.tensor([0.3, 1.25, -0.1], device=DEV)
    out, _ = P.color_transfer_idt(const, td, iterations=5, bins=32)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, const.clamp(0, 1))
    # a constant target: every map node is lo1, so the first rotation (the identity) puts every pixel on the target colour
    # (one rounding in the interpolation, one in the update: 2^-22) and every later one finds a degenerate source
    colour = torch.tensor([0.2, 0.55, 0.9], device=DEV)
    ct = torch.empty_like(td)
    ct[:] = colour
    out, _ = P.color_transfer_idt(sd, ct, iterations=5, bins=32)
    err = float((out - colour).abs().max())
    print(f'constant target: pixels end {err:.2e} from the target colour')
    assert err <= 2.0 ** -20


# ---- behaviour -------------------------------------------------------------------------------------------------------------
def compose_by_hand(P, s, t, rots, bins, rho, quantize):
    """hg_idt_run's launch sequence from the stage entry points, on slots of its own."""
    lib, st = P.lib, stream(P)
    n0, n1, iters = s.shape[0] * s.shape[1], t.shape[0] * t.shape[1], len(rots)
    sd, td, rot = torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV), dev_rot(rots)
    stride = lib.hg_idt_plane_stride(n0)
    planes = torch.empty((3, stride), device=DEV)
    m = torch.empty(3 * bins, device=DEV)
    t_rng = torch.empty(iters * 6, dtype=torch.int32, device=DEV)
    t_hist = torch.empty(iters * 3 * bins, dtype=torch.int64, device=DEV)
    s_rng, s_hist = cleared(P, 2, 3 * bins)
    out = torch.empty((n0, 3), dtype=torch.uint8 if quantize else torch.float32, device=DEV)
    P.check(lib.hg_idt_target_tables(td.data_ptr(), n1, 3, 1, rot.data_ptr(), iters, bins, t_rng.data_ptr(), t_hist.data_ptr(), st),
            'hg_idt_target_tables')
    P.check(lib.hg_idt_range(sd.data_ptr(), n0, 3, 1, rot.data_ptr(), 1, s_rng.data_ptr(), planes.data_ptr(), st), 'hg_idt_range')
    for i in range(iters):
        cur, nxt = s_rng[6 * (i & 1):], s_rng[6 * ((i + 1) & 1):]
        last = i + 1 == iters
        P.check(lib.hg_idt_hist(planes.data_ptr(), n0, 1, stride, rot[i].data_ptr(), 1, bins, cur.data_ptr(), s_hist.data_ptr(), 0,
                                st), 'hg_idt_hist')
        P.check(lib.hg_idt_table(s_hist.data_ptr(), t_hist[i * 3 * bins:].data_ptr(), t_rng[6 * i:].data_ptr(), bins, m.data_ptr(),
                                 nxt.data_ptr(), 1, st), 'hg_idt_table')
        P.check(lib.hg_idt_apply(planes.data_ptr(), n0, rot[i].data_ptr(), None if last else rot[i + 1].data_ptr(), bins,
                                 cur.data_ptr(), m.data_ptr(), rho, nxt.data_ptr(), out.data_ptr(), int(quantize), st), 'hg_idt_apply')
    return out.reshape(s.shape)


@pytest.mark.parametrize('bins,iters,rho,quantize', [(32, 6, 1.0, False), (64, 3, 0.6, True), (1024, None, 1.0, False)])
def test_run_equals_the_stages_composed_by_hand_bit_for_bit(P, bins, iters, rho, quantize):
    if iters is None:
        iters = P.lib.hg_idt_target_chunk(bins) + 1               # the target's counters take two histogram launches
    s, t = R.seeded_pair('bimodal')
    rots = R.rotations(iters, seed=9)
    sd, td = torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV)
    a, _ = P.color_transfer_idt(sd, td, bins=bins, relaxation=rho, rotations=rots, quantize=quantize)
    b, _ = P.color_transfer_idt(sd, td, bins=bins, relaxation=rho, rotations=rots, quantize=quantize)
    c = compose_by_hand(P, s, t, rots, bins, rho, quantize)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert np.array_equal(sd.cpu().numpy(), s) and np.array_equal(td.cpu().numpy(), t)           # the inputs are only read


def test_quantize_truncates_the_float_output(P):
    s, t = R.seeded_pair('smooth')
    sd, td = torch.from_numpy(s).to(DEV), torch.from_numpy(t * 2.0 - 0.5).to(DEV)               # far outside [0, 1]: it clips
    f, _ = P.color_transfer_idt(sd, td, iterations=5, bins=32)
    q, _ = P.color_transfer_idt(sd, td, iterations=5, bins=32, quantize=True)
    assert q.dtype == torch.uint8 and q.shape == f.shape and torch.equal(q, (f * 255.0).to(torch.uint8))
    assert float(f.min()) == 0.0 and float(f.max()) == 1.0 and int(q.max()) == 255 and int(q.min()) == 0


@pytest.mark.parametrize('kind', ['smooth', 'bimodal'])
def test_self_transfer_is_the_identity(P, kind):
    _, t = R.seeded_pair(kind)
    img = torch.from_numpy(t * 1.2 - 0.1).to(DEV)                  # partly outside [0, 1]: the output is clipped
    out, _ = P.color_transfer_idt(img, img, iterations=ITERS, bins=32)
    err = float((out - img.clamp(0, 1)).abs().max())
    print(f'self-transfer ({kind}, {ITERS} rotations): |out - clip(in)| = {err:.2e} (bar {2.0 ** -20:.2e})')
    assert err <= 2.0 ** -20


def test_idt_is_closer_to_a_bimodal_target_than_mkl(P):
    s, t = R.seeded_pair('bimodal')
    sd, td = torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV)
    ho = R.held_out()
    idt, _ = P.color_transfer_idt(sd, td, iterations=ITERS, bins=32)
    mkl, _ = P.color_transfer_mkl(sd, td)
    w_idt, w_mkl = R.sliced_w1(idt.cpu().numpy(), t, ho), R.sliced_w1(mkl.cpu().numpy(), t, ho)
    print(f'held-out sliced W1 to the bimodal target: before {R.sliced_w1(s, t, ho):.4f}, MKL {w_mkl:.4f}, IDT {w_idt:.4f}')
    assert w_idt < w_mkl


def test_python_surface_refusals_on_the_device(P):
    from histogan_amd._lib import HgError
    x = torch.rand(6, 7, 3, device=DEV)
    with pytest.raises(ValueError, match=r'color_transfer_idt: source must be an \(H, W, 3\) image'):
        P.color_transfer_idt(torch.rand(6, 7, 4, device=DEV), x)
    with pytest.raises(ValueError, match=r'rotations must be \(iterations, 3, 3\)'):
        P.color_transfer_idt(x, x, rotations=np.eye(3))
    for kw, word in ((dict(bins=1), 'bins'), (dict(bins=P.lib.hg_idt_max_bins() + 1), 'LDS'), (dict(relaxation=0.0), 'relaxation'),
                     (dict(relaxation=1.5), 'relaxation')):
        with pytest.raises(HgError, match=word):
            P.color_transfer_idt(x, x, iterations=2, **kw)


# ---- recoloringTrainer.evaluate --------------------------------------------------------------------------------------------
def test_evaluate_post_recoloring_idt(P, tmp_path, monkeypatch):
    torch.manual_seed(0)
    from ReHistoGAN.rehistoGAN import recoloringTrainer
    tr = recoloringTrainer('idt', str(tmp_path / 'results'), str(tmp_path / 'models'), image_size=64, network_capacity=4,
                           batch_size=1, hist_bin=16, hist_insz=32)
    tr.init_GAN()
    rs = np.random.RandomState(4)
    photo = np.clip(0.5 + 0.25 * np.sin(np.mgrid[0:40, 0:52][0][..., None] / 6.0 + np.arange(3)) + rs.normal(0, 0.05, (40, 52, 3)),
                    0, 1)
    photo = np.round(photo * 255) / 255                             # (H, W, 3) float64 in [0, 1], as evaluate receives it
    img = torch.rand(1, 3, 64, 64, device=DEV)
    h = torch.rand(1, 3, 16, 16, device=DEV)
    h = h / h.sum(dim=(1, 2, 3), keepdim=True)
    writes = []
    real = P.save_rgb
    monkeypatch.setattr(P, 'save_rgb', lambda a, p: (writes.append(a.clone()), real(a, p)))
    src = torch.from_numpy(np.ascontiguousarray(photo, dtype=np.float32)).to(DEV)
    outs = {}
    for mode in ('idt', True):
        with torch.no_grad():
            g = tr.evaluate(f'out_{mode}', image_batch=img, hist_batch=h, original_image=photo, save_input=False,
                            post_recoloring=mode)
        assert len(writes) == 1 and writes[0].dtype == torch.uint8 and writes[0].shape == (40, 52, 3)
        fn = P.color_transfer_idt if mode == 'idt' else P.color_transfer_mkl
        assert torch.equal(writes[0], fn(src, g[0].permute(1, 2, 0), quantize=True)[0])    # True: the linear map, as before
        outs[mode] = (writes.pop(), g)
    # on one generated image the two transfers differ
    g = outs['idt'][1]
    assert not torch.equal(outs['idt'][0], P.color_transfer_mkl(src, g[0].permute(1, 2, 0), quantize=True)[0])
    with pytest.raises(ValueError, match='post_recoloring'):
        tr.evaluate('bad', image_batch=img, hist_batch=h, original_image=photo, post_recoloring='nonsense')
