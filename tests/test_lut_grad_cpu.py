"""CPU-side checks of the differentiable 3D LUTs (hg_lut_apply_bwd, hg_lut_adam_step, include/hg_lut.h version 118;
post.lut_apply(differentiable=True), lut_smoothness, lut_adam_step, lut_refine; evaluate(post_recoloring='lut_refine')): the
reference tests/lut_grad_ref.py against the properties its definition promises, the host side of the C ABI and of the Python
surface, and the conditions on the inputs that the GPU tests rely on.  No kernel is launched.

Before the feature the ABI tests fail for want of the symbols and of version 118, the surface tests for want of the keyword and
the functions.

Measured here: the reference refine loop of the issue's setup (48^2 image, N = 9, h = 32, trilinear, lr 5e-3, lambda 0, from the
identity) goes 0.3384 -> 0.2229 (10 steps) -> 0.1533 (50): 0.453 of the initial loss."""
import ctypes
import types

import numpy as np
import pytest
import torch

import lut_grad_ref as G
import lut_ref as R

EINVAL, EWORKSPACE, ESIZE, EPIXELS = -1, -4, -27, -28
INTERPOLATIONS = ('tetrahedral', 'trilinear')


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


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interpolation', INTERPOLATIONS)
def test_reference_backward_is_the_adjoint_of_apply(interpolation):
    """apply is linear in the LUT where nothing is clipped: <g, J dL> = <J^T g, dL>, in fp64 up to round-off."""
    n, rs = 5, np.random.RandomState(1)
    lut = (0.25 + 0.5 * rs.rand(n, n, n, 3))                                   # entries in [0.25, 0.75]: no output is clipped
    x = rs.rand(700, 3).astype(np.float32)
    g, dl = rs.randn(700, 3).astype(np.float32).astype(np.float64), rs.randn(n, n, n, 3)        # g is fp32 in the ABI
    t = 1e-3
    val = G.pieces(x, lut, interpolation)[0]
    assert val.min() > 0.2 and val.max() < 0.8
    jdl = (R.apply(x, lut + t * dl, interpolation) - R.apply(x, lut - t * dl, interpolation)) / (2 * t)
    _, glut = G.backward(x, lut, g, interpolation)
    lhs, rhs = float((g * jdl).sum()), float((glut * dl).sum())
    print(f'{interpolation}: <g, J dL> = {lhs:.12e}, <J^T g, dL> = {rhs:.12e}')
    assert abs(lhs - rhs) <= 1e-9 * max(abs(lhs), 1.0)
    # the weights of every pixel sum to one
    om = G.pieces(x, lut, interpolation)[3]
    assert np.abs(om.sum(1) - 1).max() <= 1e-15 and om.min() >= -2.0 ** -17 and om.max() <= 1 + 2.0 ** -17


@pytest.mark.parametrize('interpolation', INTERPOLATIONS)
def test_reference_gx_matches_central_differences_inside_the_cells(interpolation):
    n, rs = 5, np.random.RandomState(2)
    lut = R.random_lut(n, 5).astype(np.float64)
    x = (np.rint(rs.rand(3000, 3) * 2.0 ** 16) / 2.0 ** 16).astype(np.float32)
    step = 2.0 ** -12                                                           # x +- step is exact in fp32
    keep = G.comparable(x, n, margin=4 * step * (n - 1))
    x, g = x[keep], rs.randn(int(keep.sum()), 3).astype(np.float32).astype(np.float64)
    assert len(x) > 1500
    val = G.pieces(x, lut, interpolation)[0]
    # the clip does not switch inside the step: |d val / d x| <= (n - 1) * 2 = 8 per axis, 8 * step = 2e-3
    inside = ((val > 0.01) & (val < 0.99)) | (val < -0.01) | (val > 1.01)
    g = np.where(inside, g, 0.0)
    gx, _ = G.backward(x, lut, g, interpolation)
    num = np.zeros_like(gx)
    for c in range(3):
        e = np.zeros(3, dtype=np.float32)
        e[c] = step
        num[:, c] = (g * (R.apply(x + e, lut, interpolation) - R.apply(x - e, lut, interpolation))).sum(1) / (2.0 * step)
    err = np.abs(gx - num).max()
    print(f'{interpolation}: max |gx - central difference| {err:.2e} over {len(x)} pixels, max |gx| {np.abs(gx).max():.2f}')
    # both interpolants are affine along one axis inside a cell (and a tetrahedron): the difference quotient is exact up to round-off
    assert err <= 1e-8 * max(1.0, np.abs(gx).max())


def test_reference_masks_and_integer_scatter():
    n = 4
    lut = R.random_lut(n, 2)
    x = G.gx_image(n, 3, 600)
    g = np.random.RandomState(0).randn(600, 3).astype(np.float32)
    g[5, 1], g[6, 0], g[7, 2] = np.nan, np.inf, -np.inf
    for interpolation in INTERPOLATIONS:
        gx, glut = G.backward(x, lut, g, interpolation)
        assert np.isfinite(gx).all() and np.isfinite(glut).all()
        assert np.all(gx[~G.input_mask(x)] == 0) and np.all(gx[90, 0] == 0) and gx[92, 1] == 0
        bits, sums, counts, gl32, u = G.int_scatter(x, lut, g, interpolation)
        finite = np.abs(g[np.isfinite(g)])
        assert np.float32(finite.max()).view(np.uint32) == bits and finite.max() < u * 2.0 ** G.GRAD_BITS <= 2 * finite.max()
        err = np.abs(gl32.astype(np.float64) - glut)
        bar = counts * u / 2 + 2.0 ** -24 * np.abs(glut)
        print(f'{interpolation}: integer scatter against fp64: max err {err.max():.2e}, largest err / bar {np.max(err / np.maximum(bar, 1e-300)):.3f}')
        assert np.all(err <= bar)
        assert np.array_equal(G.int_scatter(x[::-1], lut, g[::-1], interpolation)[1], sums)      # no sum depends on its order
    z = G.int_scatter(x, lut, np.zeros_like(g))
    assert z[0] == 0 and not z[1].any() and not z[3].any()
    assert G.gmax_bits(np.array([np.nan, np.inf], dtype=np.float32)) == 0
    assert (1 << G.GRAD_BITS) * G.MAX_PIXELS <= 1 << 62


def test_smoothness_and_its_gradient(P):
    for n in (2, 3, 9):
        lut = torch.from_numpy(R.random_lut(n, n).astype(np.float64)).requires_grad_(True)
        r = P.lut_smoothness(lut)
        want = G.smoothness(lut.detach().numpy())
        assert r.dim() == 0 and abs(float(r.detach()) - want) <= 1e-12 * want
        r.backward()
        formula = G.smoothness_grad(lut.detach().numpy(), ident=R.identity(n))
        err = np.abs(lut.grad.numpy() - formula).max()
        print(f'N = {n}: R = {want:.6f}, max |autograd - formula| {err:.2e}')
        assert err <= 1e-12 * np.abs(formula).max()
    assert float(P.lut_smoothness(P.lut_identity(7, device='cpu'))) == 0.0
    shifted = P.lut_identity(7, device='cpu') + 0.25                               # a constant displacement costs nothing
    assert float(P.lut_smoothness(shifted)) <= 1e-12
    scaled = P.lut_identity(5, device='cpu').double() * 1.5                        # d = x / 2: |grad d|^2 = 1 / 4 per channel
    assert abs(float(P.lut_smoothness(scaled)) - 0.25) <= 1e-12
    with pytest.raises(ValueError, match='lut must'):
        P.lut_smoothness(torch.zeros(3, 3, 3))


def test_reference_adam_step_is_torch_adam():
    n, rs = 3, np.random.RandomState(0)
    lut, m, v = R.random_lut(n, 1).astype(np.float64), np.zeros((n, n, n, 3)), np.zeros((n, n, n, 3))
    p = torch.from_numpy(lut.copy()).requires_grad_(True)
    opt = torch.optim.Adam([p], lr=5e-3, betas=G.BETAS, eps=G.EPS)
    for step in (1, 2, 3):
        grad = rs.randn(n, n, n, 3)
        p.grad = torch.from_numpy(grad.copy())
        opt.step()
        lut, m, v = G.adam_step(lut, grad, m, v, step, 5e-3, 0.0)
        assert np.abs(lut - p.detach().numpy()).max() <= 1e-14
    with_reg = G.adam_step(lut, np.zeros_like(lut), m * 0, v * 0, 1, 5e-3, 0.3)[0]
    direction = -np.sign(G.smoothness_grad(lut))
    assert np.array_equal(np.sign(with_reg - lut), direction)


# ---- the C ABI, host side --------------------------------------------------------------------------------------------------------
def test_abi_queries_and_refusals_before_any_launch(L):
    lib = L.lib
    assert lib.hg_version() >= 118
    for name, nargs in (('hg_lut_apply_bwd', 15), ('hg_lut_adam_step', 13), ('hg_lut_grad_lds_n', 0), ('hg_lut_grad_max_pixels', 0),
                        ('hg_lut_grad_blocks', 1), ('hg_lut_grad_workspace_bytes', 1)):
        assert name in L.EXPORTS and len(getattr(lib, name).argtypes) == nargs, name
    lds_n = lib.hg_lut_grad_lds_n()
    assert lds_n == 17 and lds_n ** 3 * 3 * 8 <= 160 * 1024 < (lds_n + 2) ** 3 * 3 * 8
    assert lib.hg_lut_grad_max_pixels() == 1 << 26 == G.MAX_PIXELS
    assert lib.hg_lut_grad_blocks(1) == 1 and lib.hg_lut_grad_blocks(4096) == 1 and lib.hg_lut_grad_blocks(4097) == 2
    assert lib.hg_lut_grad_blocks(1 << 26) == 256 and lib.hg_lut_grad_blocks((1 << 26) + 1) == 0 and lib.hg_lut_grad_blocks(0) == 0
    for n in (2, 17, 33, 65):
        assert lib.hg_lut_grad_workspace_bytes(n) >= 16 + n ** 3 * 24 and lib.hg_lut_grad_workspace_bytes(n) % 16 == 0
    assert lib.hg_lut_grad_workspace_bytes(1) == 0 and lib.hg_lut_grad_workspace_bytes(66) == 0
    assert b'2^26' in lib.hg_error_string(EPIXELS)

    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)          # never dereferenced: every call returns before a launch
    ws = lib.hg_lut_grad_workspace_bytes(17)
    def bw(x=p, u8=0, n=10, ps=3, cs=1, lut=p, N=17, tri=0, g=p, gx=p, glut=p, wsp=p, nbytes=ws, blocks=0):
        return lib.hg_lut_apply_bwd(x, u8, n, ps, cs, lut, N, tri, g, gx, glut, wsp, nbytes, blocks, None)
    for kw in (dict(u8=1), dict(x=None), dict(lut=None), dict(g=None), dict(gx=None, glut=None), dict(n=0), dict(ps=0), dict(cs=-1),
               dict(blocks=-1), dict(blocks=513), dict(wsp=None), dict(wsp=ctypes.c_void_p(4104)), dict(g=odd), dict(gx=odd),
               dict(glut=odd), dict(lut=odd)):
        assert bw(**kw) == EINVAL, kw
    assert bw(N=1) == ESIZE and bw(N=66) == ESIZE
    assert bw(n=(1 << 26) + 1) == EPIXELS
    assert bw(nbytes=ws - 1) == EWORKSPACE and bw(N=33) == EWORKSPACE

    def ad(lin=p, grad=p, m=p, v=p, lout=ctypes.c_void_p(8192), N=9, lam=0.1, lr=5e-3, b1=0.9, b2=0.999, eps=1e-8, step=1):
        return lib.hg_lut_adam_step(lin, grad, m, v, lout, N, lam, lr, b1, b2, eps, step, None)
    for kw in (dict(lin=None), dict(grad=None), dict(m=None), dict(v=None), dict(lout=None), dict(lout=p), dict(step=0),
               dict(lr=float('nan')), dict(lr=float('inf')), dict(lam=float('nan')), dict(lam=float('inf')), dict(lam=-1e-3),
               dict(b1=1.0), dict(b2=-0.1), dict(eps=float('nan')), dict(eps=-1.0), dict(grad=odd)):
        assert ad(**kw) == EINVAL, kw
    assert ad(N=1) == ESIZE and ad(N=66) == ESIZE


# ---- the Python surface refuses before a device is touched ----------------------------------------------------------------------
def test_python_surface_value_errors_and_cpu_refusal(P):
    import inspect
    img, lut = torch.rand(8, 9, 3), torch.rand(5, 5, 5, 3)
    assert inspect.signature(P.lut_apply).parameters['differentiable'].default is False
    with pytest.raises(ValueError, match='differentiable'):
        P.lut_apply(torch.zeros(8, 9, 3, dtype=torch.uint8), lut, differentiable=True)
    with pytest.raises(ValueError, match='differentiable'):
        P.lut_apply(img, lut, quantize=True, differentiable=True)
    with pytest.raises(RuntimeError, match='lut_apply.*no CPU implementation'):
        P.lut_apply(img, lut, differentiable=True)
    with pytest.raises(ValueError, match='image must'):
        P.lut_apply(torch.rand(3, 8, 9), lut, differentiable=True)
    with pytest.raises(ValueError, match='grad must'):
        P.lut_apply_backward(img, lut, torch.rand(9, 8, 3))
    with pytest.raises(ValueError, match='nothing to compute'):
        P.lut_apply_backward(img, lut, img, want_image=False, want_lut=False)
    from histogram_classes.RGBuvHistBlock import RGBuvHistBlock
    block = RGBuvHistBlock(h=16, device='cpu')
    hist = torch.rand(1, 3, 16, 16)
    for kw, match in ((dict(steps=-1), 'steps'), (dict(steps=2.5), 'steps'), (dict(lr=0.0), 'lr must'), (dict(lr=float('nan')), 'lr must'),
                      (dict(lr=float('inf')), 'lr must'), (dict(lambda_smooth=-1e-3), 'lambda_smooth'),
                      (dict(lambda_smooth=float('nan')), 'lambda_smooth'), (dict(lambda_smooth=float('inf')), 'lambda_smooth'),
                      (dict(interpolation='nearest'), 'interpolation'), (dict(weight=torch.rand(9, 8)), 'weight must')):
        with pytest.raises(ValueError, match=match):
            P.lut_refine(lut, img, hist, block, **kw)
    with pytest.raises(ValueError, match='target_hist'):
        P.lut_refine(lut, img, torch.rand(2, 3, 16, 16), block)
    with pytest.raises(ValueError, match='hist_block'):
        P.lut_refine(lut, img, hist, lambda x: x)
    with pytest.raises(ValueError, match='lut must'):
        P.lut_refine(torch.rand(5, 5, 5), img, hist, block)
    with pytest.raises(RuntimeError, match='lut_refine.*no CPU implementation'):
        P.lut_refine(lut, img, hist, block)
    z = torch.zeros(5, 5, 5, 3)
    with pytest.raises(ValueError, match='step must'):
        P.lut_adam_step(lut, z, z.clone(), z.clone(), 0)
    with pytest.raises(ValueError, match='lr must'):
        P.lut_adam_step(lut, z, z.clone(), z.clone(), 1, lr=float('nan'))
    with pytest.raises(ValueError, match='out must not'):
        P.lut_adam_step(lut, z, z.clone(), z.clone(), 1, out=lut)
    with pytest.raises(RuntimeError, match='lut_adam_step.*no CPU implementation'):
        P.lut_adam_step(lut, z, z.clone(), z.clone(), 1)
    assert P.LUT_GRAD_MAX_PIXELS == G.MAX_PIXELS and (P.LUT_ADAM_BETAS, P.LUT_ADAM_EPS) == (G.BETAS, G.EPS)
    assert P.LUT_REFINE_STEPS > 0 and 0 < P.LUT_REFINE_LR < 1 and P.LUT_REFINE_LAMBDA >= 0
    # the working copy: what the block would make of the image
    big = torch.rand(40, 52, 3) * 1.5 - 0.25
    small_block = RGBuvHistBlock(h=16, insz=32, device='cpu')
    work, w = P.lut_working_copy(big, small_block, torch.rand(40, 52))
    assert work.shape == (32, 32, 3) and w.shape == (32, 32) and work.min() >= 0 and work.max() <= 1
    same, none = P.lut_working_copy(img, small_block)
    assert none is None and torch.equal(same, img)
    assert torch.equal(small_block(work.permute(2, 0, 1)[None]), small_block(big.permute(2, 0, 1)[None]))
    assert 'lut_refine' in P.__doc__ and 'differentiable' in P.lut_apply.__doc__


def test_evaluate_names_the_lut_refine_mode():
    import inspect
    from histogan_amd.retrainer import recoloringTrainer
    with pytest.raises(ValueError, match="post_recoloring=.*'lut'.*'lut_refine'"):
        recoloringTrainer.evaluate(types.SimpleNamespace(), post_recoloring='lut_refined')
    assert "post_recoloring='lut_refine'" in recoloringTrainer.evaluate.__doc__
    assert 'refine' not in ' '.join(inspect.signature(recoloringTrainer.evaluate).parameters)


# ---- conditions on the inputs of the GPU tests ------------------------------------------------------------------------------------
def test_standard_inputs_keep_every_output_away_from_the_clip():
    """On lut_ref.random_lut(n, n) and lut_ref.apply_image(n, seed=n) the unclipped value of every pixel stays at least 1e-5
    from 0 and from 1, so fp32 and fp64 agree on every output mask (tests/test_lut_grad_gpu.py asserts it again)."""
    for n in (2, 3, 5, 17, 18, 33):
        x = R.apply_image(n, seed=n).reshape(-1, 3)
        for interpolation in INTERPOLATIONS:
            val = G.pieces(x, R.random_lut(n, n), interpolation)[0]
            dist = np.minimum(np.abs(val), np.abs(val - 1)).min()
            print(f'N = {n} {interpolation}: distance of the unclipped values to the clip {dist:.2e}')
            assert dist >= 1e-5


def test_gx_generator_keeps_the_uncompared_share_small():
    for n in (2, 3, 17, 33):
        x = G.gx_image(n, seed=n)
        for interpolation in INTERPOLATIONS:
            share = 1.0 - G.gx_comparable(x, R.random_lut(n, n), interpolation).mean()
            print(f'N = {n} {interpolation}: {100 * share:.2f} % of the gx pixels are checked for finiteness only')
            assert share <= 0.05
        assert (~G.input_mask(x)).any(1).sum() >= 20 and not np.isfinite(x).all()


@pytest.fixture(scope='module')
def refine_setup():
    img = R.smooth_image(48, 1).astype(np.float32)
    return img, G.target_histogram(R.true_map(img), 32)


def test_reference_refine_loop_reaches_the_target(refine_setup):
    """The issue's setup: N = 9, h = 32, trilinear, lr 5e-3, lambda 0, 50 steps from the identity.  Bar: 0.6 of the initial loss."""
    img, target = refine_setup
    _, losses = G.refine(R.identity(9), img, target, 32, 50, 5e-3, 0.0, 'trilinear')
    print('reference refine losses at steps 0, 1, 2, 5, 10, 50:', ' '.join(f'{losses[k]:.4f}' for k in (0, 1, 2, 5, 10, 50)))
    assert losses[50] <= 0.6 * losses[0]
    assert np.all(np.diff(losses[:11]) < 0)
