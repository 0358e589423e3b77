"""Per-pixel weighted (masked) histograms, `device='cpu'` path (histogan_amd/hist_cpu.py) and host glue.  No GPU.

Pins, under the bars of tests/test_hist_cpu_path.py (forward 1e-5, gradient 1e-4, max-norm relative):
* binary mask, no resize: a histogram is a sum over pixels, so block(x, weight=mask) equals the ORACLE (the reference's
  arithmetic, unmodified) on any image made of exactly the selected pixels, and the gradient at the selected pixels the
  oracle's autograd gradient of that image; elsewhere it is exactly 0;
* Lab block with intensity_scale: its weight is channel 0, so block(x, weight=w) equals the oracle on x with channel 0
  replaced by the fp32 product w * clamp(x0, 0, 1) -- fractional weights against the reference's arithmetic;
* fractional weights with resizing: a double-precision statement of the definition (tests/hist_weight_ref.py)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from conftest import relmax
from hist_weight_ref import (BWD_TOL, FWD_TOL, definition_fwd_bwd, gather_selected, make_block, oracle_hist, random_mask,
                             sample_image)

METHODS = [('thresholding', {}), ('RBF', dict(sigma=0.05)), ('inverse-quadratic', dict(sigma=0.02))]
PROJECTIONS = [('rgbuv', {}), ('rgbuv', dict(green_only=True)), ('rgchroma', {}), ('direct', {})]
PIN_CASES = [(proj, dict(method=m, intensity_scale=i, h=16, insz=64, **mkw, **pkw))
             for m, mkw in METHODS for proj, pkw in PROJECTIONS for i in (True, False)]


def pin_binary_mask(proj, kw, device, B=1, H=40, W=48, a=30, b=32, seed=3):
    """Returns (forward error, gradient error, max |gradient| outside the mask) of block(x, weight=mask) against the oracle
    on the gathered pixels."""
    g = torch.Generator().manual_seed(seed)
    x = sample_image(B, 3, H, W, g)
    mask = random_mask(B, H, W, a * b, g)
    blk = make_block(proj, device, **kw)
    xg = x.clone().to(device).requires_grad_(True)
    out = blk(xg, weight=mask.to(device))
    go = torch.randn(out.shape, generator=g)
    out.backward(go.to(device))
    xo = gather_selected(x, mask, a, b).detach().clone().requires_grad_(True)
    ref = oracle_hist(xo, proj, **kw)
    assert out.shape == ref.shape and out.dtype == torch.float32
    e_f = relmax(out.detach().cpu().numpy(), ref.detach().numpy())
    gx = xg.grad.cpu()
    outside = float((gx * (1 - mask).unsqueeze(1)).abs().max())
    assert torch.isfinite(gx).all()
    if ref.requires_grad:
        ref.backward(go)
        e_b = relmax(gather_selected(gx, mask, a, b).numpy(), xo.grad.numpy())
    else:                                  # thresholding without intensity scale: the reference has no gradient path
        e_b = float(gx.abs().max())
    return e_f, e_b, outside


@pytest.mark.parametrize('proj,kw', PIN_CASES)
def test_cpu_binary_mask_equals_oracle_on_the_selected_pixels(proj, kw):
    e_f, e_b, outside = pin_binary_mask(proj, kw, 'cpu')
    print(f'cpu mask pin {proj} {kw}: fwd {e_f:.2e} grad {e_b:.2e}')
    assert e_f <= FWD_TOL and e_b <= BWD_TOL
    assert outside == 0.0


def pin_lab_fractional(method, mkw, device, seed=5):
    from oracle import rgbuv_hist as O
    g = torch.Generator().manual_seed(seed)
    x = sample_image(2, 3, 36, 44, g)
    w = torch.rand(2, 1, 36, 44, generator=g)
    kw = dict(method=method, intensity_scale=True, h=16, insz=64, **mkw)
    blk = make_block('direct', device, **kw)
    xg = x.clone().to(device).requires_grad_(True)
    out = blk(xg, weight=w.to(device))
    go = torch.randn(out.shape, generator=g)
    out.backward(go.to(device))
    xo = x.clone().requires_grad_(True)
    xmod = torch.cat([w * torch.clamp(xo[:, :1], 0, 1), xo[:, 1:]], dim=1)          # fp32 product in channel 0
    ref = O.plane_hist(xmod, 'direct', **kw)
    ref.backward(go)
    return relmax(out.detach().cpu().numpy(), ref.detach().numpy()), relmax(xg.grad.cpu().numpy(), xo.grad.numpy())


@pytest.mark.parametrize('method,mkw', METHODS)
def test_cpu_lab_block_fractional_weight_equals_oracle_on_scaled_channel0(method, mkw):
    e_f, e_b = pin_lab_fractional(method, mkw, 'cpu')
    print(f'cpu lab pin {method}: fwd {e_f:.2e} grad {e_b:.2e}')
    assert e_f <= FWD_TOL and e_b <= BWD_TOL


# fractional weights / resizing / weight layouts: (projection, block kwargs, input (B, C, H, W), weight layout, pre_relu)
DEF_CASES = [
    ('rgbuv', dict(h=32, insz=24, resizing='interpolation', method='inverse-quadratic', sigma=0.02), (2, 3, 40, 56), 'b1hw', False),
    ('rgbuv', dict(h=16, insz=24, resizing='sampling', method='inverse-quadratic', sigma=0.05), (3, 4, 40, 56), 'bhw', False),
    ('rgbuv', dict(h=16, insz=30, resizing='interpolation', method='thresholding'), (2, 3, 48, 40), 'strided', False),
    ('rgbuv', dict(h=16, insz=20, resizing='sampling', method='thresholding', intensity_scale=False), (2, 3, 48, 40), 'bhw', False),
    ('rgbuv', dict(h=16, insz=64, method='RBF', sigma=0.05), (2, 3, 40, 48), 'strided', True),
    ('rgbuv', dict(h=24, insz=32, resizing='interpolation', method='RBF', sigma=0.4, hist_boundary=[-2.0, 3.0]), (2, 3, 40, 56), 'b1hw', False),
    ('rgbuv', dict(h=16, insz=64, method='inverse-quadratic', sigma=0.02, green_only=True), (2, 3, 40, 48), 'bhw', True),
    ('rgchroma', dict(h=16, insz=24, resizing='interpolation', method='inverse-quadratic', sigma=0.02, intensity_scale=True), (2, 3, 40, 56), 'strided', False),
    ('direct', dict(h=16, insz=24, resizing='sampling', method='RBF', sigma=0.05, intensity_scale=True), (2, 3, 40, 56), 'b1hw', False),
    ('direct', dict(h=16, insz=64, method='thresholding', intensity_scale=False), (2, 3, 40, 48), 'bhw', False),
]


def make_weight(layout, B, H, W, gen):
    """Real weights in [0, 1] (with exact zeros and ones), a different map per image, in the given layout."""
    w = torch.rand(B, H, W, generator=gen)
    w[:, :4] = 0.0
    w[:, -4:] = 1.0
    if layout == 'b1hw':
        return w.unsqueeze(1).contiguous()
    if layout == 'strided':                        # a non-contiguous view: every second element of a wider buffer
        buf = torch.zeros(B, H, 2 * W)
        buf[:, :, ::2] = w
        return buf[:, :, ::2]
    return w


def check_definition(proj, kw, shape, layout, pre_relu, device, seed=9):
    g = torch.Generator().manual_seed(seed)
    x = sample_image(*shape, g)
    w = make_weight(layout, shape[0], shape[2], shape[3], g)
    blk = make_block(proj, device, **kw)
    xg = x.clone().to(device).requires_grad_(True)
    wd = w.to(device)
    if layout == 'strided' and device != 'cpu':    # keep the view non-contiguous on the device too
        buf = torch.zeros(shape[0], shape[2], 2 * shape[3], device=device)
        buf[:, :, ::2] = w.to(device)
        wd = buf[:, :, ::2]
        assert not wd.is_contiguous()
    out = blk(xg, pre_relu=True, weight=wd) if pre_relu else blk(xg, weight=wd)
    go = torch.randn(out.shape, generator=g)
    out.backward(go.to(device))
    ref, gref = definition_fwd_bwd(x, w.reshape(shape[0], shape[2], shape[3]), go, projection=proj, pre_relu=pre_relu, **kw)
    e_f = relmax(out.detach().cpu().numpy(), ref)
    if np.abs(gref).max() > 0:
        e_b = relmax(xg.grad.cpu().numpy(), gref)
    else:
        e_b = float(xg.grad.abs().max())
    if shape[1] > 3:
        assert float(xg.grad[:, 3:].abs().max()) == 0.0
    return e_f, e_b


@pytest.mark.parametrize('proj,kw,shape,layout,pre_relu', DEF_CASES)
def test_cpu_fractional_weights_and_resizing_match_the_definition(proj, kw, shape, layout, pre_relu):
    e_f, e_b = check_definition(proj, kw, shape, layout, pre_relu, 'cpu')
    print(f'cpu definition {proj} {kw} {layout}: fwd {e_f:.2e} grad {e_b:.2e}')
    assert e_f <= FWD_TOL and e_b <= BWD_TOL


@pytest.mark.parametrize('proj,kw', [('rgbuv', dict(h=16, insz=24, method='inverse-quadratic')),
                                     ('rgbuv', dict(h=16, insz=64, method='thresholding')),
                                     ('rgchroma', dict(h=16, insz=64, method='RBF', sigma=0.05, intensity_scale=True)),
                                     ('direct', dict(h=16, insz=24, resizing='sampling', intensity_scale=True))])
def test_cpu_exactness_properties(proj, kw):
    g = torch.Generator().manual_seed(1)
    x = sample_image(2, 3, 40, 48, g)
    blk = make_block(proj, 'cpu', **kw)

    def run(weight):
        xr = x.clone().requires_grad_(True)
        out = blk(xr) if weight is None else blk(xr, weight=weight)
        go = torch.randn(out.shape, generator=torch.Generator().manual_seed(2))
        if out.requires_grad:
            out.backward(go)
        return out.detach(), (xr.grad if xr.grad is not None else torch.zeros_like(x))

    h0, g0 = run(None)
    h1, g1 = run(torch.ones(2, 40, 48))
    assert torch.equal(h0, h1) and torch.equal(g0, g1)                      # ones == None, bit for bit
    hz, gz = run(torch.zeros(2, 1, 40, 48))
    assert float(hz.abs().max()) == 0.0 and float(gz.abs().max()) == 0.0 and torch.isfinite(gz).all()
    w = torch.rand(2, 40, 48, generator=g) * 3 - 1                          # values outside [0, 1] behave as clamped
    ha, ga = run(w)
    hb, gb = run(w.clamp(0, 1))
    assert torch.equal(ha, hb) and torch.equal(ga, gb)


def test_cpu_weight_argument_errors():
    x = torch.rand(2, 3, 20, 24)
    for proj in ('rgbuv', 'rgchroma', 'direct'):
        blk = make_block(proj, 'cpu', h=8, insz=32)
        with pytest.raises(ValueError, match='requires grad'):
            blk(x, weight=torch.rand(2, 20, 24, requires_grad=True))
        for bad in (torch.rand(2, 24, 20), torch.rand(1, 20, 24), torch.rand(2, 3, 20, 24), torch.rand(20, 24)):
            with pytest.raises(ValueError, match='weight must have shape'):
                blk(x, weight=bad)
        assert blk(x, weight=torch.ones(2, 20, 24, dtype=torch.float64)).shape[0] == 2     # other float types are converted
    assert not torch.cuda.is_initialized(), 'the CPU path initialised the GPU'


def test_forward_signatures_document_the_extension():
    from histogram_classes.LabHistBlock import LabHistBlock
    from histogram_classes.RGBuvHistBlock import RGBuvHistBlock
    from histogram_classes.rgChromaHistBlock import rgChromaHistBlock
    from histogan_amd import hist as HH
    sig = inspect.signature(RGBuvHistBlock.forward)
    assert list(sig.parameters) == ['self', 'x', 'pre_relu', 'weight'] and sig.parameters['weight'].default is None
    for cls in (LabHistBlock, rgChromaHistBlock):
        sig = inspect.signature(cls.forward)
        assert list(sig.parameters) == ['self', 'x', 'weight'] and sig.parameters['weight'].default is None
    assert list(inspect.signature(HH.rgbuv_hist).parameters) == ['x', 'cfg', 'pre_relu', 'weight']
    assert inspect.signature(HH.run_block).parameters['weight'].default is None


def test_abi_weight_fields_and_struct_size_guard():
    """hg_hist_params grew by the weight pointer and its three strides (version 103); the struct-size guard rejects the
    previous layout's size and any other; NULL weight = no map whatever the strides say; a zero stride (broadcast) is
    accepted, a misaligned pointer is not."""
    from histogan_amd import build
    build.build()
    import histogan_amd._lib as L
    assert L.lib.hg_version() >= 103
    names = [f[0] for f in L.HgHistParams._fields_]
    assert names[-5:] == ['proj_cache', 'weight', 'weight_stride_b', 'weight_stride_h', 'weight_stride_w']
    size = ctypes.sizeof(L.HgHistParams)
    assert L.HgHistParams.weight.offset == L.HgHistParams.proj_cache.offset + 8 and size == L.HgHistParams.weight.offset + 32

    def q(**kw):
        p = L.HgHistParams()
        p.struct_size = size
        p.B, p.C, p.H, p.W = 2, 3, 16, 16
        p.stride_b, p.stride_c, p.stride_h, p.stride_w = 3 * 256, 256, 16, 1
        p.Hs, p.Ws, p.resize_mode = 16, 16, 0
        p.h, p.lo, p.hi, p.method, p.sigma = 64, -3.0, 3.0, 2, 0.02
        p.intensity_scale = 1
        for k, v in kw.items():
            setattr(p, k, v)
        f, b = ctypes.c_size_t(), ctypes.c_size_t()
        return L.lib.hg_rgbuv_hist_workspace_bytes(ctypes.byref(p), ctypes.byref(f), ctypes.byref(b)), f.value, b.value

    base = q()
    assert base[0] == 0
    assert q(struct_size=size - 16)[0] == -1 and q(struct_size=size - 32)[0] == -1 and q(struct_size=size + 8)[0] == -1
    assert q(weight=0, weight_stride_b=-7, weight_stride_h=1 << 40, weight_stride_w=3) == base        # NULL: strides unread
    assert q(weight=0x1000, weight_stride_b=256, weight_stride_h=16, weight_stride_w=1) == base       # no extra workspace
    assert q(weight=0x1000, weight_stride_b=0, weight_stride_h=16, weight_stride_w=1)[0] == 0         # broadcast over the batch
    assert q(weight=0x1002, weight_stride_b=256, weight_stride_h=16, weight_stride_w=1)[0] == -1      # misaligned


def test_alpha_weight_option_needs_transparent(tmp_path):
    from PIL import Image
    from histogan_amd.data import FolderData
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / 'a.png')
    with pytest.raises(ValueError, match='transparent'):
        FolderData(str(tmp_path), lambda x: x, 1, 8, torch.device('cpu'), transparent=False, hist_alpha_weight=True)
    ds = FolderData(str(tmp_path), lambda x: x, 1, 8, torch.device('cpu'), transparent=False)
    assert ds.alpha_weight is False


def test_cpu_folderdata_alpha_weighted_targets(tmp_path):
    """An RGBA image whose transparent half is painted a saturated colour: with hist_alpha_weight the target histogram is
    the histogram of the opaque half alone (the binary-mask pin), without it the paint counts."""
    from PIL import Image
    from histogan_amd.data import FolderData
    from oracle import rgbuv_hist as O
    rs = np.random.RandomState(0)
    img = np.zeros((24, 32, 4), np.uint8)
    img[..., :3] = rs.randint(0, 256, (24, 32, 3))
    img[:, 16:, :3] = (255, 64, 128)      # inside the histogram's [-3, 3] log-chroma range
    img[:, :16, 3] = 255
    img[:, 16:, 3] = 0
    Image.fromarray(img, 'RGBA').save(tmp_path / 'a.png')
    blk = make_block('rgbuv', 'cpu', h=16, insz=64)
    opaque = torch.from_numpy(img[:, :16, :3].astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0)
    ref = O.rgbuv_hist(opaque, h=16, insz=64).numpy()
    on = FolderData(str(tmp_path), blk, 1, 8, torch.device('cpu'), transparent=True, test=True, hist_alpha_weight=True)
    off = FolderData(str(tmp_path), blk, 1, 8, torch.device('cpu'), transparent=True, test=True)
    h_on, h_off = next(on)['histograms'].numpy(), next(off)['histograms'].numpy()
    assert relmax(h_on, ref) <= FWD_TOL
    assert relmax(h_off, ref) > 1e-2


def test_generated_alpha_as_weight_handles_fully_transparent_images():
    """The trainer's weight map for the generator-side histogram: the generated alpha, clamped and detached; an image whose
    alpha is nowhere positive (its histogram would be all zero, where the Hellinger loss has no finite gradient) is
    weighed uniformly."""
    from histogan_amd.trainer import _alpha_weight
    img = torch.rand(3, 4, 8, 8, requires_grad=True)
    with torch.no_grad():
        img[0, 3] = -0.2                   # fully transparent
        img[1, 3, :4] = -1.0               # half transparent
        img[2, 3] = 1.7                    # beyond 1
    w = _alpha_weight(img)
    assert w.shape == (3, 8, 8) and not w.requires_grad
    assert torch.equal(w[0], torch.ones(8, 8))
    assert torch.equal(w[1], img[1, 3].detach().clamp(0, 1)) and float(w[1, :4].abs().max()) == 0.0
    assert torch.equal(w[2], torch.ones(8, 8))
