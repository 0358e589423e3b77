"""`LabHistBlock(from_rgb=True)`: the sRGB -> CIE Lab projection (HG_PROJ_LAB of include/hg_hist.h), the parts that need no GPU --
the reference helper against literature values, the `device='cpu'` path (histogan_amd/hist_cpu.py, projection 'lab') against
the helper, the host-only answers of the C ABI for projection = 3, and the refusal of the stand-alone conversions to
differentiate.  Bars: forward 1e-5, gradient 1e-4, max-norm relative (tests/test_hist_planes_gpu.py)."""
import ctypes
import itertools

import pytest
import torch

import lab_ref as R
from conftest import relmax
from test_oracle_planes_golden import load as load_plane


def _block(**kw):
    from histogram_classes.LabHistBlock import LabHistBlock
    return LabHistBlock(device='cpu', **kw)


def test_helper_matches_literature_lab_values():
    assert R.check_anchors() <= 1e-3
    # and its inverse undoes it
    x = torch.rand(3, 500, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    assert float((R.lab_to_srgb(R.srgb_to_lab(x)) - x).abs().max()) <= 1e-12


def test_gamut_lies_inside_the_default_boundary():
    g = torch.linspace(0, 1, 33, dtype=torch.float64)
    lab = R.srgb_to_lab(torch.cartesian_prod(g, g, g).t())
    assert 0.0 <= float(lab[0].min()) and float(lab[0].max()) <= 1.0 + 1e-12
    assert 0.16 < float(lab[1].min()) and float(lab[1].max()) < 0.89
    assert 0.07 < float(lab[2].min()) and float(lab[2].max()) < 0.88


def test_from_rgb_false_is_the_module_as_it_was():
    g = load_plane('direct_iq_h16_sampling')
    kw = dict(g['kwargs'])
    outs = []
    for extra in ({}, {'from_rgb': False}):
        x = torch.from_numpy(g['x']).requires_grad_(True)
        out = _block(**kw, **extra)(x)
        assert relmax(out.detach().numpy(), g['hist']) <= 1e-5
        out.backward(torch.from_numpy(g['grad_out']))
        assert relmax(x.grad.numpy(), g['grad_x']) <= 1e-4
        outs.append((out.detach(), x.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert _block(from_rgb=True)._config().projection == 'lab' and _block()._config().projection == 'direct'


CPU_CASES = [
    ((2, 3, 20, 28), dict(h=16, intensity_scale=False)),
    ((2, 3, 20, 28), dict(h=16, intensity_scale=True)),
    ((1, 3, 37, 53), dict(h=16, insz=24, intensity_scale=True)),
    ((1, 3, 45, 70), dict(h=16, insz=32, resizing='sampling', intensity_scale=True)),
]


@pytest.mark.parametrize('shape,kw', CPU_CASES)
def test_cpu_path_matches_the_definition(shape, kw):
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(*shape, generator=gen)
    go = torch.rand(shape[0], 1, kw['h'], kw['h'], generator=gen)
    ref, ref_gx, _ = R.fwd_bwd(x, go, **kw)
    xr = x.clone().requires_grad_(True)
    out = _block(from_rgb=True, **kw)(xr)
    assert out.dtype == torch.float32 and out.device.type == 'cpu'
    e_f = relmax(out.detach().numpy(), ref)
    out.backward(go)
    e_b = relmax(xr.grad.numpy(), ref_gx)
    print(f'cpu lab {shape} {kw}: fwd {e_f:.2e} bwd {e_b:.2e}')
    assert e_f <= R.FWD_TOL and e_b <= R.BWD_TOL


def test_cpu_path_weight_map_and_its_gradient():
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(2, 3, 20, 28, generator=gen)
    go = torch.rand(2, 1, 16, 16, generator=gen)
    w = torch.rand(2, 1, 20, 28, generator=gen) * 1.4 - 0.2
    ref, ref_gx, ref_gw = R.fwd_bwd(x, go, w=w, weight_grad=True, h=16, intensity_scale=True)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    out = _block(from_rgb=True, h=16, intensity_scale=True)(xr, weight=wr, weight_grad=True)
    out.backward(go)
    assert relmax(out.detach().numpy(), ref) <= R.FWD_TOL
    assert relmax(xr.grad.numpy(), ref_gx) <= R.BWD_TOL and relmax(wr.grad.numpy(), ref_gw) <= R.BWD_TOL
    assert bool((wr.grad[(w < 0) | (w > 1)] == 0).all())


# ---- host-only C ABI ---------------------------------------------------------------------------------------------------
def _params(L, projection, method, h, resize, wmap, intensity=1):
    p = L.HgHistParams()
    p.struct_size = ctypes.sizeof(L.HgHistParams)
    Hs, Ws = (40, 48) if resize != 2 else (h, h)
    H, W = (Hs, Ws) if resize == 0 else (2 * Hs + 1, 2 * Ws + 3)
    p.B, p.C, p.H, p.W, p.Hs, p.Ws, p.resize_mode = 2, 3, H, W, Hs, Ws, resize
    p.stride_b, p.stride_c, p.stride_h, p.stride_w = 3 * H * W, H * W, W, 1
    p.row_idx = p.col_idx = 0x1000 if resize == 2 else None
    p.h, p.lo, p.hi, p.method, p.sigma, p.intensity_scale = h, 0.0, 1.0, method, 0.02, intensity
    p.projection = projection
    if wmap:
        p.weight = 0x2000
        p.weight_stride_b, p.weight_stride_h, p.weight_stride_w = H * W, W, 1
    return p


def _answers(L, p, weight_grad):
    ref, lib = ctypes.byref, L.lib
    f, b, n = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    r = L.HgHistRoute(struct_size=ctypes.sizeof(L.HgHistRoute))
    rc = (lib.hg_rgbuv_hist_route(ref(p), int(weight_grad), ref(r)), lib.hg_rgbuv_hist_workspace_bytes(ref(p), ref(f), ref(b)),
          lib.hg_rgbuv_hist_bwd_w_workspace_bytes(ref(p), ref(n)) if weight_grad else 0, lib.hg_rgbuv_hist_uses_proj_cache(ref(p)))
    return rc, tuple(getattr(r, k) for k, _ in L.HgHistRoute._fields_[1:]), f.value, b.value, n.value


def test_cabi_projection_3_validates_and_answers_like_direct():
    from histogan_amd import _lib as L
    assert L.lib.hg_version() >= 107 and L.HG_PROJ['lab'] == 3
    f = ctypes.c_size_t(0)
    for proj, want in ((3, 0), (4, -1), (-1, -1)):
        p = _params(L, proj, 2, 16, 0, False)
        assert L.lib.hg_rgbuv_hist_workspace_bytes(ctypes.byref(p), ctypes.byref(f), None) == want
        assert (L.lib.hg_rgbuv_hist_uses_proj_cache(ctypes.byref(p)) >= 0) == (want == 0)
    seen_fwd, seen_bwd = set(), set()
    for method, h, resize, (wmap, wgrad), intensity in itertools.product((0, 1, 2), (16, 64, 128, 130, 142), (0, 1, 2),
                                                                         ((False, False), (True, False), (True, True)), (0, 1)):
        lab = _answers(L, _params(L, 3, method, h, resize, wmap, intensity), wgrad)
        direct = _answers(L, _params(L, 2, method, h, resize, wmap, intensity), wgrad)
        assert lab == direct, (method, h, resize, wmap, wgrad, intensity, lab, direct)
        assert lab[0][0] == 0 and lab[0][1] == 0
        seen_fwd.add(L.HG_ROUTE_FWD[lab[1][0]])
        seen_bwd.add(L.HG_ROUTE_BWD[lab[1][1]])
    # the routes of DESIGN.md section 4's "one-plane projection" rows, all reached by this grid
    assert seen_fwd == {'DENSE', 'THR_SCATTER', 'RBF_SCATTER'}
    assert seen_bwd == {'PLANES', 'GENERIC', 'THR_GATHER', 'RBF_GATHER'}


def test_histconfig_lab():
    from histogan_amd.hist import HistConfig
    c = HistConfig(projection='lab')
    assert (c.lo, c.hi, c.projection) == (0.0, 1.0, 'lab')
    with pytest.raises(ValueError):
        HistConfig(projection='xyz')


def test_standalone_conversions_refuse_to_differentiate():
    from histogan_amd import post
    x = torch.rand(1, 3, 4, 4, requires_grad=True)          # a CPU tensor: the check comes before anything touches HIP
    for fn in (post.srgb_to_lab, post.lab_to_srgb):
        with pytest.raises(ValueError, match='from_rgb=True'):
            fn(x)
