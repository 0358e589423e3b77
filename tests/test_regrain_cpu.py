"""CPU-side checks of regrain (hg_regrain_*, include/hg_regrain.h; post.regrain, post.regrain_levels;
recoloringTrainer.evaluate(post_recoloring='idt_regrain')): the host side of the C ABI and of the Python surface, and the
fp64 reference tests/regrain_ref.py against the properties its definition promises.  No kernel is launched.

Before the feature the ABI tests fail for want of the symbols and of version 117, the Python-surface tests for want of the
functions and of evaluate's fifth mode, and the reference's tests for want of post.REGRAIN_RHO and post.REGRAIN_MIN_SIDE."""
import ctypes
import inspect
import types

import numpy as np
import pytest
import torch

import regrain_ref as R

EINVAL, ESIZE, EITERATIONS, ESMOOTHNESS, EMINSIDE = -1, -29, -30, -31, -32
SIZES = [(2, 2), (2, 3), (3, 5), (21, 21), (40, 41), (41, 41), (42, 40), (42, 43), (96, 128), (673, 673), (3000, 4000), (1345, 700)]


@pytest.fixture(scope='module')
def L():
    from histogan_amd import build
    build.build()
    import histogan_amd._lib as L
    return L


@pytest.fixture(scope='module')
def P(L):
    from histogan_amd import post
    return post


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def test_abi_exports_version_and_constants(L, P):
    lib = L.lib
    assert lib.hg_version() >= 117
    for name in ('hg_regrain_begin', 'hg_regrain_coef', 'hg_regrain_sweep', 'hg_regrain_finish', 'hg_regrain_levels',
                 'hg_regrain_workspace_bytes', 'hg_regrain_plan_fused', 'hg_regrain_max_fused', 'hg_regrain_tile_h',
                 'hg_regrain_tile_w', 'hg_regrain_sweep_launches', 'hg_regrain_check'):
        assert name in L.EXPORTS and hasattr(lib, name)
    th, tw, kmax = lib.hg_regrain_tile_h(), lib.hg_regrain_tile_w(), lib.hg_regrain_max_fused()
    assert th >= 8 and tw >= 8 and tw % 4 == 0 and kmax >= 2 and kmax == P.REGRAIN_MAX_FUSED
    # the staged region of the deepest fusion -- six fp32 planes, the columns' halo rounded up to 4 -- fits the 160 KiB of a CU
    assert (th + 2 * kmax) * (tw + 2 * ((kmax + 3) // 4 * 4)) * 4 * 6 <= 160 * 1024
    assert P.REGRAIN_RHO == R.RHO == 0.2 and P.REGRAIN_MIN_SIDE == R.MIN_SIDE == 20 and P.REGRAIN_ITERATIONS == R.ITERATIONS
    for n in (1, 4, 5, 64):
        for k in range(1, kmax + 1):
            assert lib.hg_regrain_sweep_launches(n, k) == -(-n // k)
    assert lib.hg_regrain_sweep_launches(0, 1) == 0 and lib.hg_regrain_sweep_launches(4, 0) == 0
    assert lib.hg_regrain_sweep_launches(4, kmax + 1) == 0
    for h, w in SIZES:
        for n in (1, 4, 64):
            assert 1 <= lib.hg_regrain_plan_fused(h, w, n) <= kmax
    assert lib.hg_regrain_plan_fused(1, 8, 4) == 0 and lib.hg_regrain_plan_fused(8, 8, 0) == 0
    # the measured plan: one launch of n sweeps from n = 4 on, 8 per launch above, one sweep per launch below
    assert [lib.hg_regrain_plan_fused(3000, 4000, n) for n in (1, 3, 4, 6, 16, 64)] == [1, 1, 4, 6, 8, 8]
    for code, word in ((ESIZE, b'2'), (EITERATIONS, b'iterations'), (ESMOOTHNESS, b'smoothness'), (EMINSIDE, b'min_side')):
        msg = lib.hg_error_string(code)
        assert b'regrain' in msg and word in msg


def test_levels_agree_between_library_python_and_reference(L, P):
    lib = L.lib
    for h, w in SIZES:
        for its in (R.ITERATIONS, (4,), (4, 16), (1,) * 12):
            for min_side in (1, 2, 20, 21):
                want = R.levels(h, w, its, min_side)
                assert P.regrain_levels(h, w, its, min_side) == want
                assert lib.hg_regrain_levels(h, w, len(its), min_side) == len(want)
                assert all(a >= 2 and b >= 2 for a, b in want)
                nb = lib.hg_regrain_workspace_bytes(h, w, len(want))
                assert nb == 4 * R.workspace_floats(want) and nb % 16 == 0
    count = lambda h, w: lib.hg_regrain_levels(h, w, 6, 20)  # noqa: E731
    assert (count(2, 2), count(21, 21), count(41, 41), count(42, 40), count(42, 43), count(673, 673)) == (1, 1, 2, 1, 2, 6)
    assert lib.hg_regrain_levels(673 * 4, 673 * 4, 6, 20) == 6 and lib.hg_regrain_levels(673 * 4, 673 * 4, 8, 20) == 8
    assert len(R.levels(9, 7, R.ITERATIONS, 1)) == 3 and len(R.levels(9, 7, R.ITERATIONS, 2)) == 2    # (5, 4), (3, 2): 2 > 2 fails
    # refused arguments: no level, no workspace
    for args in ((1, 8, 6, 20), (8, 1, 6, 20), (0, 0, 6, 20), (-4, 8, 6, 20), (8, 8, 0, 20), (8, 8, 6, 0), (1 << 15, 1 << 14, 6, 20)):
        assert lib.hg_regrain_levels(*args) == 0, args
    for args in ((1, 8, 1), (8, 1, 1), (8, 8, 0), (8, 8, 4), (8, 8, 32), (1 << 15, 1 << 14, 1), (-1, -1, 1)):
        assert lib.hg_regrain_workspace_bytes(*args) == 0, args
    with pytest.raises(ValueError, match='regrain_levels'):
        P.regrain_levels(1, 8)
    with pytest.raises(ValueError, match='min_side'):
        P.regrain_levels(8, 8, (4,), 0)


def test_every_refusal_comes_from_the_host_checks(L):
    lib = L.lib
    chk = lambda H=8, W=8, n=6, s=1.0, m=20: lib.hg_regrain_check(H, W, n, s, m)  # noqa: E731
    assert chk() == 0
    assert chk(H=1) == ESIZE and chk(W=1) == ESIZE and chk(H=1 << 15, W=(1 << 13) + 1) == ESIZE
    assert chk(n=0) == EITERATIONS and chk(n=-3) == EITERATIONS
    for s in (0.0, -1.0, float('inf'), float('nan'), 1e-60, 1e60):
        assert chk(s=s) == ESMOOTHNESS, s
    assert chk(m=0) == EMINSIDE and chk(m=-20) == EMINSIDE and chk(m=1) == 0

    # never dereferenced: every call below returns before a launch.  The regions are far enough apart for an 8 x 8 level.
    q = lambda k: ctypes.c_void_p(1 << 20 | k << 12)  # noqa: E731
    odd = ctypes.c_void_p((1 << 20) + 2)

    def begin(o=q(0), ops=3, ocs=1, t=q(1), tps=3, tcs=1, H=8, W=8, I=q(2), E=q(3)):
        return lib.hg_regrain_begin(o, ops, ocs, t, tps, tcs, H, W, I, E, None)
    for kw in (dict(o=None), dict(t=None), dict(I=None), dict(E=None), dict(ops=0), dict(ocs=-1), dict(tps=0), dict(tcs=0),
               dict(o=odd), dict(E=odd), dict(E=q(2))):
        assert begin(**kw) == EINVAL, kw
    assert begin(H=1) == ESIZE and begin(W=1) == ESIZE and begin(H=0, W=0) == ESIZE

    def coef(I=q(0), H=8, W=8, level=0, s=1.0, c=q(1), scratch=q(2)):
        return lib.hg_regrain_coef(I, H, W, level, s, c, scratch, None)
    for kw in (dict(I=None), dict(c=None), dict(scratch=None), dict(level=-1), dict(level=31), dict(c=odd), dict(scratch=q(1)),
               dict(c=q(0))):
        assert coef(**kw) == EINVAL, kw
    assert coef(H=1) == ESIZE and coef(s=0.0) == ESMOOTHNESS and coef(s=float('nan')) == ESMOOTHNESS and coef(s=-2.0) == ESMOOTHNESS

    kmax = lib.hg_regrain_max_fused()

    def sweep(a=q(0), b=q(1), E=q(2), c=q(3), H=8, W=8, n=4, fused=1):
        return lib.hg_regrain_sweep(a, b, E, c, H, W, n, fused, None)
    for kw in (dict(a=None), dict(b=None), dict(E=None), dict(c=None), dict(fused=-1), dict(fused=kmax + 1), dict(a=odd),
               dict(b=q(0)), dict(b=ctypes.c_void_p((1 << 20) + 16)), dict(E=q(0)), dict(E=q(1)), dict(c=q(0)), dict(c=q(1))):
        assert sweep(**kw) == EINVAL, kw                           # aliased or overlapping source and destination among them
    assert sweep(H=1) == ESIZE and sweep(W=0) == ESIZE and sweep(n=0) == EITERATIONS and sweep(n=-1, fused=2) == EITERATIONS

    def finish(I=q(0), D=q(1), H=8, W=8, out=q(2), quant=0):
        return lib.hg_regrain_finish(I, D, H, W, out, quant, None)
    for kw in (dict(I=None), dict(D=None), dict(out=None), dict(out=odd), dict(D=odd)):
        assert finish(**kw) == EINVAL, kw
    assert finish(H=1) == ESIZE and finish(W=1, quant=1) == ESIZE


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_regrain_refuses_bad_arguments_with_value_errors(P):
    a, b = torch.rand(6, 5, 3), torch.rand(6, 5, 3)
    with pytest.raises(ValueError, match='one size'):
        P.regrain(a, torch.rand(6, 4, 3))
    with pytest.raises(ValueError, match='one device'):
        P.regrain(a, torch.empty(6, 5, 3, device='meta'))
    for shape in ((1, 5, 3), (5, 1, 3), (1, 1, 3)):
        with pytest.raises(ValueError, match='at least 2 x 2'):
            P.regrain(torch.rand(shape), torch.rand(shape))
    for bad in ((3, 6, 5), (6, 5), (6, 5, 4)):
        with pytest.raises(ValueError, match=r'\(H, W, 3\)'):
            P.regrain(torch.rand(bad), torch.rand(bad))
    with pytest.raises(ValueError, match=r'\(H, W, 3\)'):
        P.regrain(torch.zeros(6, 5, 3, dtype=torch.uint8), b)
    for its in ((), [], (0,), (4, -1), (4, 0, 8), (2.5,), (True,), None, 4):
        with pytest.raises(ValueError, match='iterations'):
            P.regrain(a, b, iterations=its)
    for s in (0, 0.0, -1.0, float('inf'), float('nan'), 1e-60, 'soft', None):
        with pytest.raises(ValueError, match='smoothness'):
            P.regrain(a, b, smoothness=s)
    for m in (0, -1, 2.5, None):
        with pytest.raises(ValueError, match='min_side'):
            P.regrain(a, b, min_side=m)
    for f in (-1, P.REGRAIN_MAX_FUSED + 1, 1.0, True):
        with pytest.raises(ValueError, match='fused'):
            P.regrain(a, b, fused=f)
    with pytest.raises(RuntimeError, match='no CPU implementation'):           # valid arguments: only the device is missing
        P.regrain(a, b)
    sig = inspect.signature(P.regrain)
    assert list(sig.parameters) == ['original', 'transferred', 'iterations', 'smoothness', 'min_side', 'quantize', 'fused']
    assert sig.parameters['iterations'].default == (4, 16, 32, 64, 64, 64) and sig.parameters['smoothness'].default == 1.0
    assert sig.parameters['min_side'].default == 20 and sig.parameters['quantize'].default is False and sig.parameters['fused'].default == 0
    assert list(inspect.signature(P.color_transfer_idt).parameters) == ['source', 'target', 'iterations', 'bins', 'relaxation',
                                                                        'rotations', 'seed', 'quantize']
    assert 'regrain' in P.__doc__


def test_evaluate_names_the_regrain_mode(P):
    from histogan_amd.retrainer import recoloringTrainer
    for bad in ('nonsense', 'LUT', 'cube', '', 'regrain', 'idt-regrain', 'IDT_REGRAIN'):
        with pytest.raises(ValueError, match="post_recoloring=.*'idt'.*'palette'.*'lut'.*'idt_regrain'"):
            recoloringTrainer.evaluate(types.SimpleNamespace(), post_recoloring=bad)
    assert "post_recoloring='idt_regrain'" in recoloringTrainer.evaluate.__doc__
    assert list(inspect.signature(recoloringTrainer.evaluate).parameters) == [
        'self', 'num', 'image_batch', 'hist_batch', 'triple_hist', 'double_hist', 'resizing', 'resizing_method', 'swapping_levels',
        'pyramid_levels', 'level_blending', 'original_size', 'input_image_name', 'original_image', 'post_recoloring', 'save_input']


# ---- properties of the reference -----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pair():
    I, T = R.synthetic_pair()
    I.setflags(write=False)
    T.setflags(write=False)
    return I, T


def test_reference_identities(P, pair):
    """T = I gives E = 0, D = 0 at every level and J = I exactly; T = I + c gives D = c up to rounding: the update is a convex
    combination of E = c and D = c with weights that sum to 1 within a few ulp (measured: 1.1e-16)."""
    I, _ = pair
    assert np.array_equal(R.regrain(I, I), I)
    assert np.array_equal(R.regrain(I, I, iterations=(1, 1), min_side=2), I)
    for c in (0.03125, -0.07, 0.2):
        assert np.max(np.abs(R.regrain(I, I + c, clip=False) - (I + c))) <= 1e-12


def test_reference_maximum_principle(pair):
    """Every sweep is a convex combination of E(p), D(p) and D's neighbours, so D started inside [min E, max E] stays there per
    channel.  Slack: s is the rounded (1 - rho) / den, so the weights sum to 1 within 8 ulp, per sweep."""
    I, T = pair
    Ip, E = R.begin(I, T)
    for level in (0, 2):
        C = R.coef(Ip, level)
        lo, hi = E.min(axis=(1, 2), keepdims=True), E.max(axis=(1, 2), keepdims=True)
        D = E.copy()
        for n in range(1, 41):
            D = R.sweep_once(D, E, C)
            slack = 8 * n * 2.0 ** -53 * np.abs(E).max()
            assert np.all(D >= lo - slack) and np.all(D <= hi + slack), (level, n)
    assert np.all(R.coef(Ip, 0)[3] > 0) and np.all(R.coef(Ip, 0)[0] >= 0)


@pytest.mark.parametrize('k', [1, 2, 5, 8])
def test_reference_window_sweeps_equal_global_sweeps_on_the_interior(pair, k):
    """What the tiled kernel relies on: k sweeps on a window cropped with a margin of k pixels (clipped at the image's border),
    its border cells taking nothing from outside the window, equal the global sweeps on the window's interior, bit for bit."""
    I, T = pair
    Ip, E = R.begin(I, T)
    C = R.coef(Ip, 0)
    H, W = E.shape[1:]
    D0 = E + 0.01 * np.sin(np.arange(H * W).reshape(H, W))
    want = R.sweep(D0, E, C, k)
    for y0, y1, x0, x1 in ((0, 17, 0, 23), (30, 51, 40, 77), (H - 9, H, W - 13, W), (0, H, 50, 60), (40, 41, 0, W)):
        ya, yb, xa, xb = max(y0 - k, 0), min(y1 + k, H), max(x0 - k, 0), min(x1 + k, W)
        got = R.sweep(D0[:, ya:yb, xa:xb], E[:, ya:yb, xa:xb], C[:, ya:yb, xa:xb], k)
        assert np.array_equal(got[:, y0 - ya:y1 - ya, x0 - xa:x1 - xa], want[:, y0:y1, x0:x1])
    if k > 1:       # and one pixel less of margin is not enough
        got = R.sweep(D0[:, 30 - k + 1:51 + k, 40:77], E[:, 30 - k + 1:51 + k, 40:77], C[:, 30 - k + 1:51 + k, 40:77], k)
        assert not np.array_equal(got[:, k - 1:k - 1 + 21, :], want[:, 30:51, 40:77])


def test_reference_float32_run_follows_the_float64_run(pair):
    I, T = (v.astype(np.float32) for v in pair)
    J32, J64 = R.regrain(I, T, dtype=np.float32), R.regrain(I, T)
    assert J32.dtype == np.float32 and J64.dtype == np.float64
    assert np.max(np.abs(J32 - J64)) <= 64 * 2.0 ** -24             # measured 1.8e-7


# ---- the effect --------------------------------------------------------------------------------------------------------------
def test_reference_restores_the_gradients_and_keeps_the_colours(pair):
    """The 96 x 128 synthetic pair (ramps, a hard-edged patch; T an affine colour map of I quantised to 24 levels plus
    sigma = 0.01 noise), defaults: three levels.  Measured with regrain_ref in fp64: rms(grad J - grad I) / rms(grad T - grad I)
    = 0.052 (cap 0.2), mean |J - T| = 0.0139 against mean |T - I| = 0.0560."""
    I, T = pair
    assert R.levels(*I.shape[:2]) == [(96, 128), (48, 64), (24, 32)]
    J = R.regrain(I, T)
    ratio = R.gradient_rms(J, I) / R.gradient_rms(T, I)
    print(f'gradient mismatch ratio {ratio:.4f}; mean|J-T| {np.abs(J - T).mean():.4f}; mean|T-I| {np.abs(T - I).mean():.4f}')
    assert ratio <= 0.2
    assert np.abs(J - T).mean() < np.abs(T - I).mean()
