"""CPU-side checks of the iterative distribution transfer (hg_idt_*, include/hg_post.h; post.color_transfer_idt,
post.idt_rotations; recoloringTrainer.evaluate(post_recoloring='idt')): the rotations, the fp64 reference of tests/idt_ref.py
against the properties its definition promises, and the host side of the C ABI and of the Python surface.  No kernel is
launched.

Before the feature the ABI tests fail for want of the symbols and of version 113, and the Python-surface tests for want of
post.idt_rotations, post.color_transfer_idt and of evaluate's refusal of an unknown post_recoloring string."""
import ctypes
import types

import numpy as np
import pytest
import torch

import idt_ref as R
import post_ref


@pytest.fixture(scope='module')
def L():
    from histogan_amd import build
    build.build()
    import histogan_amd._lib as L
    return L


# ---- rotations ---------------------------------------------------------------------------------------------------------
def test_rotations_are_proper_seeded_and_start_at_the_identity(L):
    from histogan_amd import post
    rot = post.idt_rotations(12, seed=3)
    assert rot.shape == (12, 3, 3) and rot.dtype == np.float64
    assert np.array_equal(rot[0], np.eye(3))
    for q in rot:
        assert np.abs(q @ q.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(q) - 1.0) <= 1e-14
    assert np.array_equal(rot, post.idt_rotations(12, seed=3)) and not np.array_equal(rot[1:], post.idt_rotations(12, seed=4)[1:])
    assert np.array_equal(rot[:5], post.idt_rotations(5, seed=3))            # a shorter schedule is a prefix
    assert np.array_equal(rot, R.rotations(12, seed=3))                      # the reference's restatement agrees
    assert np.array_equal(post.idt_rotations(20), post.idt_rotations(20, seed=0))
    with pytest.raises(ValueError, match='at least 1'):
        post.idt_rotations(0)


def test_range_encoding_preserves_order_and_round_trips(L):
    from histogan_amd import post
    vals = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 0.25, 1.7320508, np.inf], dtype=np.float32)
    enc = [int(post.idt_encode_range([v] * 3, [v] * 3)[0]) for v in vals]
    assert enc == sorted(enc) and len(set(enc)) == len(enc) and all(0 <= e <= 0xffffffff for e in enc)
    lo, hi = post.idt_decode_range(post.idt_encode_range(vals[1:4], vals[5:8]))
    assert np.array_equal(lo.view(np.uint32), vals[1:4].view(np.uint32)) and np.array_equal(hi, vals[5:8])


# ---- the reference helper ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['smooth', 'bimodal'])
def test_reference_self_transfer_moves_nothing(kind):
    _, t = R.seeded_pair(kind)
    rots = R.rotations(10)
    moved = np.abs(R.transfer(t, t, rots, 32, clip=False) - t).max()
    moved32 = np.abs(R.transfer(t, t, rots, 32, dtype=np.float32, clip=False) - t).max()
    print(f'self-transfer ({kind}): pixels move by {moved:.1e} in fp64 and {moved32:.1e} in fp32 arithmetic')
    assert moved <= 1e-14 and moved32 <= 2.0 ** -20


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_reference_histogram_conserves_every_pixel(dtype):
    s, _ = R.seeded_pair('smooth')
    for Rm in R.rotations(4, seed=2):
        v = R.project(s.reshape(-1, 3), Rm, dtype)
        lo, hi = R.ranges(v)
        for a in range(3):
            for n in (2, 7, 64, 257):
                h = R.histogram(v[:, a], lo[a], hi[a], n, dtype)
                assert h.dtype == np.int64 and h.min() >= 0 and int(h.sum()) == R.UNITS * v.shape[0]
    # a degenerate axis: everything on node 0
    h = R.histogram(np.full(10, 0.3), 0.3, 0.3, 8, dtype)
    assert int(h[0]) == 10 * R.UNITS and int(h[1:].sum()) == 0


def test_reference_map_of_equal_histograms_is_the_node_grid():
    rs = np.random.RandomState(0)
    h = rs.randint(1, 5, 40) * 1000               # every node populated: u' == k exactly
    h[0], h[-1] = 7, 9
    M = R.quantile_map(h, h, -0.5, 1.5)
    assert np.abs(M - (-0.5 + np.arange(40) / 39.0 * 2.0)).max() <= 1e-15
    # a flat stretch of the target CDF maps to its left end; a degenerate target maps everything to lo1
    h0, h1 = np.array([4, 4, 4, 4]), np.array([8, 0, 0, 8])
    assert np.allclose(R.quantile_map(h0, h1, 0.0, 3.0), [0.0, 0.0, 2.5, 3.0], atol=1e-15)
    assert np.array_equal(R.quantile_map(h0, np.array([16, 0, 0, 0]), 0.7, 0.7), np.full(4, 0.7))


@pytest.mark.parametrize('kind', ['smooth', 'bimodal'])
def test_reference_beats_the_linear_map_on_held_out_rotations(kind):
    s, t = R.seeded_pair(kind)
    ho = R.held_out()
    before = R.sliced_w1(s, t, ho)
    mkl = R.sliced_w1(post_ref.color_transfer(s, t)[0], t, ho)
    idt = R.sliced_w1(R.transfer(s, t, R.rotations(10), 32), t, ho)
    print(f'sliced W1 to the {kind} target along held-out rotations: before {before:.4f}, after MKL {mkl:.4f}, after IDT {idt:.4f}')
    assert idt < mkl < before


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
IDT_SYMBOLS = ('hg_idt_block_pixels', 'hg_idt_max_bins', 'hg_idt_group_pixels', 'hg_idt_target_chunk', 'hg_idt_blocks', 'hg_idt_plane_stride',
               'hg_idt_workspace_bytes', 'hg_idt_clear', 'hg_idt_range', 'hg_idt_hist', 'hg_idt_table', 'hg_idt_apply',
               'hg_idt_target_tables', 'hg_idt_run')
EINVAL, EWORKSPACE, EBINS, EBINS_LDS, EITER, ERELAX, EPIXELS = -1, -4, -20, -21, -22, -23, -24


def test_symbols_version_and_constants(L):
    lib = L.lib
    for name in IDT_SYMBOLS:
        assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.hg_version() >= 113
    bp, mb = lib.hg_idt_block_pixels(), lib.hg_idt_max_bins()
    assert 4 <= bp <= 65535 and bp % 4 == 0                      # 65535 pixels of 65536 units fit a uint32 counter
    assert bp * R.UNITS < 2 ** 32
    assert 3 * mb * 4 <= 64 * 1024 and mb >= 1024 and lib.hg_idt_group_pixels() == 1024
    for bins in (2, 16, 256, mb):
        c = lib.hg_idt_target_chunk(bins)
        assert c >= 1 and c * 3 * bins <= 3 * mb < (c + 1) * 3 * bins
    assert lib.hg_idt_target_chunk(1) == 0 and lib.hg_idt_target_chunk(mb + 1) == 0
    assert lib.hg_idt_blocks(1) == 1 and lib.hg_idt_blocks(0) == 0 and lib.hg_idt_blocks(2 ** 32) == 0
    assert lib.hg_idt_blocks(4032 * 3024) > 256                  # a phone photo fills the 256 CUs
    assert [lib.hg_idt_plane_stride(n) for n in (1, 4, 5, 1279)] == [4, 4, 8, 1280] and lib.hg_idt_plane_stride(0) == 0
    codes = {EBINS, EBINS_LDS, EITER, ERELAX, EPIXELS}
    strings = {lib.hg_error_string(c) for c in codes}
    assert len(strings) == len(codes) and all(b'distribution transfer' in s for s in strings)
    assert b'relaxation' in lib.hg_error_string(ERELAX) and b'bins' in lib.hg_error_string(EBINS_LDS)


def test_workspace_query(L):
    q = L.lib.hg_idt_workspace_bytes
    up16 = lambda v: (v + 15) // 16 * 16                                                                  # noqa: E731

    def want(n0, iters, bins):          # planes, map, two source range sets, target range sets, source and target counters
        return (up16(3 * ((n0 + 3) // 4 * 4) * 4) + up16(3 * bins * 4) + up16(2 * 24) + up16(iters * 24) + up16(3 * bins * 8) +
                up16(iters * 3 * bins * 8))
    for n0, n1, iters, bins in [(1, 1, 1, 2), (1279, 1024, 10, 64), (4032 * 3024, 65536, 20, 256), (5, 7, 3, 4096)]:
        assert q(n0, n1, iters, bins) == want(n0, iters, bins)
    assert q(100, 10 ** 6, 4, 16) == q(100, 1, 4, 16)              # the target is only read
    assert q(0, 8, 1, 8) == 0 and q(8, 0, 1, 8) == 0 and q(8, 8, 0, 8) == 0 and q(8, 8, 1, 1) == 0
    assert q(8, 8, 1, L.lib.hg_idt_max_bins() + 1) == 0 and q(2 ** 32, 8, 1, 8) == 0 and q(8, 2 ** 32, 1, 8) == 0


def test_every_refusal_has_its_code_and_nothing_is_launched(L):
    """The library loads without a GPU; every call below returns before it would launch, so the pointers -- never
    dereferenced on the host -- need not be real."""
    lib = L.lib
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    mb = lib.hg_idt_max_bins()
    ws = lib.hg_idt_workspace_bytes(100, 80, 5, 32)

    def run(src=p, n0=100, ps0=3, cs0=1, tgt=p, n1=80, ps1=3, cs1=1, rot=p, iters=5, bins=32, rho=1.0, out=p, u8=0, wsp=p,
            nbytes=ws):
        return lib.hg_idt_run(src, n0, ps0, cs0, tgt, n1, ps1, cs1, rot, iters, bins, rho, out, u8, wsp, nbytes, None)
    for kw in (dict(src=None), dict(tgt=None), dict(rot=None), dict(out=None), dict(wsp=None), dict(ps0=0), dict(cs1=-1),
               dict(out=odd), dict(wsp=odd)):
        assert run(**kw) == EINVAL, kw
    assert run(bins=1) == EBINS and run(bins=0) == EBINS and run(bins=-4) == EBINS
    assert run(bins=mb + 1, nbytes=1 << 40) == EBINS_LDS
    assert run(iters=0) == EITER and run(iters=-1) == EITER
    for rho in (0.0, -0.5, 1.0000001, float('nan'), float('inf')):
        assert run(rho=rho) == ERELAX, rho
    assert run(n0=0) == EPIXELS and run(n1=0) == EPIXELS and run(n0=2 ** 32, nbytes=1 << 60) == EPIXELS
    assert run(n1=2 ** 32) == EPIXELS
    assert run(nbytes=ws - 1) == EWORKSPACE and run(nbytes=0) == EWORKSPACE

    # the stage entry points
    assert lib.hg_idt_clear(None, 1, None, 0, None) == EINVAL and lib.hg_idt_clear(p, 1, None, 3, None) == EINVAL
    assert lib.hg_idt_clear(p, -1, p, 0, None) == EINVAL and lib.hg_idt_clear(None, 0, None, 0, None) == 0
    rng = lambda x=p, n=10, ps=3, cs=1, rot=p, nrot=1, r=p, pl=None: lib.hg_idt_range(x, n, ps, cs, rot, nrot, r, pl, None)   # noqa: E731
    assert rng(x=None) == EINVAL and rng(rot=None) == EINVAL and rng(r=None) == EINVAL and rng(ps=0) == EINVAL
    assert rng(pl=odd) == EINVAL and rng(nrot=0) == EITER and rng(n=0) == EPIXELS and rng(n=2 ** 32) == EPIXELS
    hist = lambda x=p, n=10, ps=3, cs=1, rot=p, nrot=1, bins=32, r=p, h=p, blocks=0: lib.hg_idt_hist(   # noqa: E731
        x, n, ps, cs, rot, nrot, bins, r, h, blocks, None)
    assert hist(x=None) == EINVAL and hist(r=None) == EINVAL and hist(h=None) == EINVAL and hist(blocks=-1) == EINVAL
    assert hist(blocks=4096) == EINVAL and hist(bins=1) == EBINS and hist(bins=mb + 1) == EBINS_LDS
    assert hist(nrot=0) == EITER and hist(nrot=lib.hg_idt_target_chunk(32) + 1) == EITER and hist(n=0) == EPIXELS
    tab = lambda h0=p, h1=p, r=p, bins=32, m=p: lib.hg_idt_table(h0, h1, r, bins, m, None, 0, None)                # noqa: E731
    assert tab(h0=None) == EINVAL and tab(h1=None) == EINVAL and tab(r=None) == EINVAL and tab(m=None) == EINVAL
    assert tab(bins=1) == EBINS and tab(bins=mb + 1) == EBINS_LDS
    app = lambda pl=p, n=10, rot=p, nxt=None, bins=32, r=p, m=p, rho=1.0, nr=None, out=p, u8=0: lib.hg_idt_apply(  # noqa: E731
        pl, n, rot, nxt, bins, r, m, rho, nr, out, u8, None)
    assert app(pl=None) == EINVAL and app(pl=odd) == EINVAL and app(rot=None) == EINVAL and app(r=None) == EINVAL
    assert app(m=None) == EINVAL and app(out=None) == EINVAL and app(out=odd) == EINVAL
    assert app(nxt=p, nr=None) == EINVAL                           # a next rotation needs the range set it reduces into
    assert app(bins=1) == EBINS and app(bins=mb + 1) == EBINS_LDS and app(rho=0.0) == ERELAX and app(rho=1.5) == ERELAX
    assert app(n=0) == EPIXELS
    tt = lambda t=p, n=10, rot=p, iters=3, bins=32, r=p, h=p: lib.hg_idt_target_tables(t, n, 3, 1, rot, iters, bins, r, h, None)  # noqa: E731
    assert tt(t=None) == EINVAL and tt(rot=None) == EINVAL and tt(r=None) == EINVAL and tt(h=None) == EINVAL
    assert tt(bins=1) == EBINS and tt(bins=mb + 1) == EBINS_LDS and tt(iters=0) == EITER and tt(n=0) == EPIXELS


# ---- the Python surface refuses before a device is touched ----------------------------------------------------------------
def test_color_transfer_idt_refuses_cpu_tensors_and_bad_shapes(L):
    from histogan_amd import post
    x = torch.rand(8, 9, 3)
    with pytest.raises(RuntimeError, match='color_transfer_idt.*no CPU implementation'):
        post.color_transfer_idt(x, x)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        post.color_transfer_idt(x, x, iterations=3, bins=16, quantize=True)
    with pytest.raises(RuntimeError, match='color_transfer_mkl.*no CPU implementation'):
        post.color_transfer_mkl(x, x)                              # the wording of the linear transfer is unchanged
    assert 'sixteenth' in post.color_transfer_idt.__doc__ and 'bins' in post.color_transfer_idt.__doc__


def test_evaluate_refuses_an_unknown_post_recoloring(L):
    from histogan_amd import project
    from histogan_amd.retrainer import recoloringTrainer
    for bad in ('nonsense', 'mkl', 'IDT', ''):
        with pytest.raises(ValueError, match="post_recoloring=.*'idt'"):
            recoloringTrainer.evaluate(types.SimpleNamespace(), post_recoloring=bad)
    assert 'color_transfer_idt' in project.__doc__ and 'color_transfer_mkl' in project.__doc__
