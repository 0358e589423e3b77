"""DiffAugment kernels (histogan_amd/csrc/hg_augment.hip) beyond their first workgroup, against oracle/diff_augment.py
evaluated in fp64 (itself pinned to the reference by tests/test_oracle_augment_golden.py).

tests/test_augment_gpu.py replays the reference's recorded draws at W, H <= 32; here the shapes are the ones at which
the kernels' grids and loops have more than one block, chunk or trip, up to the 3 x 256 x 256 sample of a training run:

  a. k_aug_spatial<ADJ>: several ragged x- and y-blocks, C != 3, every parameter at the ends of its range -- bit-exact;
  b. k_sample_sum / k_sample_mean_finish / k_aug_color<ADJ>: both sum paths with several chunks and wrapped grid-stride
     loops, the 32-chunk cap, B > 64, C in (1, 3, 4);
  c. DiffAugment's own assembly of a chain (row merge, flush rule, order of the draws) against the reference's
     sequential definition, at 8 x 3 x 256 x 256;
  d. the gradient penalty's double backward through translation -> cutout -> color;
  e. the launchers' refusals.

Every case first asserts, from its shape alone, that it reaches the structure it is there for.  Inputs come from a
seeded CPU generator and are neither constant, symmetric nor periodic, so a wrong index changes values.
"""
import json

import pytest
import torch

from conftest import relmax
from oracle import diff_augment as O

pytestmark = pytest.mark.gpu

E_FWD, E_ADJ = 2e-6, 1e-5        # the colour bars of tests/test_augment_gpu.py (relmax)
E_MEAN = 2e-6                    # per-sample mean, relative
ID = (0, 0, 0, 0, 0, 1, 0, 1, 0)


def _record(record_testsuite_property, key, val):
    """A case's measured errors as a test-suite property (kept by pytest --junitxml), and on stdout."""
    print(f'{key}: {json.dumps(val, sort_keys=True)}')
    record_testsuite_property(key, json.dumps(val, sort_keys=True))


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1009 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _row(B, **cols):
    """(B, 9) identity rows with the named columns replaced."""
    names = ('flip', 'rh', 'rw', 'sh', 'sw', 'r0', 'r1', 'c0', 'c1')
    p = torch.tensor(ID, dtype=torch.int32).repeat(B, 1)
    for k, v in cols.items():
        p[:, names.index(k)] = torch.as_tensor(v, dtype=torch.int32)
    return p


def _combined(H, W, flip):
    """flip, both rolls (one negative), both shifts (one negative) and an interior cutout in one row."""
    return (flip, H // 3, -(W // 4), -(H // 8), W // 9, H // 5, H // 2, W // 4, (2 * W) // 3)


def _spatial_parity(x, rows, names, dev):
    """augment_spatial and its adjoint against the oracle; -> the names of the samples that are not bit-equal."""
    from histogan_amd.augment import augment_spatial
    rows = torch.tensor(rows, dtype=torch.int32)
    g = _gen(*x.shape, 7)
    go = torch.randn(x.shape, generator=g)
    xg = x.to(dev).requires_grad_(True)
    y = augment_spatial(xg, rows)
    gx, = torch.autograd.grad(y, xg, go.to(dev))
    xd = x.double().requires_grad_(True)
    yd = O.spatial(xd, rows)
    gd, = torch.autograd.grad(yd, xd, go.double())
    y, gx, yr, gr = y.detach().cpu(), gx.cpu(), O.spatial(x, rows), gd.float()
    bad_f = [names[b] for b in range(x.shape[0]) if not torch.equal(y[b], yr[b])]
    bad_g = [names[b] for b in range(x.shape[0]) if not torch.equal(gx[b], gr[b])]
    return bad_f, bad_g, float((y - yr).abs().max()), float((gx - gr).abs().max())


# ---- a. spatial kernel, forward and adjoint, bit-exact ----------------------------------------------------------------
def _edge_rows(H, W, zero_shift):
    """One row per sample: every parameter at the ends of its range (include/hg_augment.h for the columns)."""
    return [
        ('identity', ID),
        ('flip', (1,) + ID[1:]),
        ('roll_end', (0, H - 1, 1, 0, 0, 1, 0, 1, 0)),
        ('roll_negative', (0, -1, -(W - 1), 0, 0, 1, 0, 1, 0)),            # augment_spatial normalises these
        ('roll_full_turn', (0, H, 2 * W, 0, 0, 1, 0, 1, 0)),               # the identity again
        ('shift_one_corner', (0, 0, 0, H - 1, -(W - 1), 1, 0, 1, 0)),      # out[0, W-1] = x[H-1, 0], zeros elsewhere
        ('shift_all_out', (0, 0, 0, H, 0, 1, 0, 1, 0) if zero_shift == 'rows' else (0, 0, 0, 0, -W, 1, 0, 1, 0)),
        ('cut_everything', (0, 0, 0, 0, 0, 0, H - 1, 0, W - 1)),
        ('cut_last_pixel', (0, 0, 0, 0, 0, H - 1, H - 1, W - 1, W - 1)),
        ('cut_nothing', (0, 0, 0, 0, 0, 5, 4, 0, W - 1)),                  # r0 > r1 although c0 <= c1
        ('combined_flip', _combined(H, W, 1)),
        ('combined', _combined(H, W, 0)),
    ]


@pytest.mark.parametrize('zero_shift', ['rows', 'cols'])
def test_spatial_edge_rows_bit_exact(zero_shift, gpu_device, record_testsuite_property):
    """(12, 3, 67, 131): 3 x-blocks and 17 y-blocks, the last of each ragged; one hand-written row per sample.  The two
    cases differ in the all-zero shift only: (H, 0) or (0, -W)."""
    B, C, H, W = 12, 3, 67, 131
    assert W > 128 and W % 64 != 0 and (H + 3) // 4 == 17 and H % 4 != 0 and W % 2 == 1
    table = _edge_rows(H, W, zero_shift)
    assert len(table) == B
    x = torch.randn(B, C, H, W, generator=_gen(B, C, H, W))
    bad_f, bad_g, e_f, e_g = _spatial_parity(x, [r for _, r in table], [n for n, _ in table], gpu_device)
    _record(record_testsuite_property, f'augment_shapes/spatial_edges/{zero_shift}', dict(fwd=e_f, adj=e_g))
    assert not bad_f and not bad_g, (bad_f, bad_g)


def test_spatial_full_blocks_five_channels_bit_exact(gpu_device, record_testsuite_property):
    """(2, 5, 256, 256): 4 full x-blocks, 64 y-blocks, C != 3 (b = blockIdx.z / C)."""
    B, C, H, W = 2, 5, 256, 256
    assert W % 64 == 0 and W // 64 == 4 and H % 4 == 0 and C != 3
    x = torch.randn(B, C, H, W, generator=_gen(B, C, H, W))
    bad_f, bad_g, e_f, e_g = _spatial_parity(x, [_combined(H, W, 1), _combined(H, W, 0)], ['combined_flip', 'combined'],
                                             gpu_device)
    _record(record_testsuite_property, 'augment_shapes/spatial_256', dict(fwd=e_f, adj=e_g))
    assert not bad_f and not bad_g, (bad_f, bad_g)


@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (1, 3, 1, 70)])
def test_spatial_single_row_of_blocks_bit_exact(shape, gpu_device, record_testsuite_property):
    """One pixel, and one image row of two x-blocks: blocks whose threads are almost all out of range."""
    B, C, H, W = shape
    assert (H + 3) // 4 == 1 and H < 4 and W % 64 != 0
    x = torch.randn(B, C, H, W, generator=_gen(B, C, H, W))
    worst = dict(fwd=0.0, adj=0.0)
    for name, row in (('flip', (1,) + ID[1:]), ('roll_negative', (0, -1, -(W - 1), 0, 0, 1, 0, 1, 0)),
                      ('combined_flip', _combined(H, W, 1))):
        bad_f, bad_g, e_f, e_g = _spatial_parity(x, [row], [name], gpu_device)
        worst = dict(fwd=max(worst['fwd'], e_f), adj=max(worst['adj'], e_g))
        assert not bad_f and not bad_g, (bad_f, bad_g)
    _record(record_testsuite_property, f'augment_shapes/spatial_{H}x{W}', worst)


# ---- b. colour kernel and the sample mean --------------------------------------------------------------------------------
def _chunks(chw):
    """The grid of k_sample_sum (hg_sample_mean)."""
    return min(max((chw // 4 + 1023) // 1024, 1), 32)


COLOR_CASES = [
    # shape, rows, what the shape must reach
    ((3, 3, 67, 131), 'drawn', lambda B, C, H, W: (C * H * W) % 4 != 0 and _chunks(C * H * W) == 7
        and C * H * W > 7 * 256 and (H * W + 255) // 256 == 35),
    ((3, 3, 67, 131), 'ends', lambda B, C, H, W: (C * H * W) % 4 != 0 and H * W > 256),
    ((2, 4, 33, 65), 'drawn', lambda B, C, H, W: C == 4 and (C * H * W) % 4 == 0 and _chunks(C * H * W) == 3),
    ((70, 3, 8, 8), 'drawn', lambda B, C, H, W: B > 64),
    ((1, 3, 37, 41), 'drawn', lambda B, C, H, W: (C * H * W) % 4 != 0 and (C * H * W // 4 + 1023) // 1024 >= 2
        and _chunks(C * H * W) == 2),
    ((2, 3, 256, 256), 'drawn', lambda B, C, H, W: (C * H * W) % 4 == 0 and C * H * W // 4 > 31 * 1024
        and _chunks(C * H * W) == 32 and -(-(C * H * W // 4) // (32 * 256)) == 6 and (H * W + 255) // 256 == 256),
    ((2, 1, 5, 7), 'drawn', lambda B, C, H, W: C == 1),
]


def _draw_color(B, g):
    """The three draws of DiffAugment's 'color': brightness in [-0.5, 0.5), saturation in [0, 2), contrast in [0.5, 1.5)."""
    return torch.stack([torch.rand(B, generator=g) - 0.5, torch.rand(B, generator=g) * 2, torch.rand(B, generator=g) + 0.5],
                       dim=1)


@pytest.mark.parametrize('shape,kind,reach', COLOR_CASES, ids=[f'{"x".join(map(str, s))}-{k}' for s, k, _ in COLOR_CASES])
def test_color_and_sample_mean_match_fp64(shape, kind, reach, gpu_device, record_testsuite_property):
    """augment_color, its gradient and the per-sample mean against the fp64 oracle: 2e-6 / 1e-5 relmax, mean 2e-6 relative."""
    from histogan_amd import augment as A
    B, C, H, W = shape
    assert reach(B, C, H, W), shape
    g = _gen(B, C, H, W, 3)
    x = torch.rand(B, C, H, W, generator=g)
    if kind == 'ends':                     # the identity, and both ends of all three ranges
        rows = torch.tensor([[0.0, 1.0, 1.0], [0.5, 0.0, 0.5], [-0.5, 2.0, 1.5]])
    else:
        rows = _draw_color(B, g)
    go = torch.randn(B, C, H, W, generator=g)
    xg = x.to(gpu_device).requires_grad_(True)
    y = A.augment_color(xg, rows)
    gx, = torch.autograd.grad(y, xg, go.to(gpu_device))
    mean = A._sample_mean(xg.detach())
    xd = x.double().requires_grad_(True)
    yd = O.color(xd, rows.double())
    gd, = torch.autograd.grad(yd, xd, go.double())
    md = x.double().mean((1, 2, 3))
    e = dict(fwd=relmax(y.detach().cpu().numpy(), yd.detach().numpy()), adj=relmax(gx.cpu().numpy(), gd.numpy()),
             mean=float(((mean.cpu().double() - md).abs() / md.abs()).max()))
    _record(record_testsuite_property, f'augment_shapes/color/{"x".join(map(str, shape))}/{kind}', e)
    if kind == 'ends':                     # row 0 is the identity map
        assert relmax(y[0].detach().cpu().numpy(), x[0].detach().numpy()) <= E_FWD
    assert e['fwd'] <= E_FWD, e
    assert e['adj'] <= E_ADJ, e
    assert e['mean'] <= E_MEAN, e


# ---- c. the chain as DiffAugment assembles it, at training resolution ----------------------------------------------------
CHAIN_SHAPE = (8, 3, 256, 256)
CHAINS = [
    # types, per-sample flip, launches of the spatial kernel
    (['offset', 'translation', 'cutout'], True, 1),
    (['translation', 'cutout', 'color'], False, 1),
    (['cutout', 'translation'], False, 2),
    (['color', 'offset_h', 'color'], False, 1),
]


@pytest.fixture(scope='module')
def chain_input():
    g = _gen(*CHAIN_SHAPE)
    x = torch.rand(CHAIN_SHAPE, generator=g)
    return x, torch.randn(CHAIN_SHAPE, generator=g), torch.randint(0, 2, (CHAIN_SHAPE[0],), generator=g)


def _redraw(types, flip, B, H, W, g):
    """The chain's parameters drawn again, in the order DiffAugment consumes its generator, as ONE step per augmentation:
    the reference applies them one at a time, in the order named (utils/diff_augment.py:9-13)."""
    from histogan_amd import augment as A
    steps = [] if flip is None else [('spatial', _row(B, flip=flip))]
    for t in types:
        if t == 'color':
            steps.append(('color', _draw_color(B, g)))
        elif t in ('offset', 'offset_h', 'offset_v'):
            vh, vv = A.draw_offset(B, H, W, 1, 0 if t == 'offset_v' else 1, 0 if t == 'offset_h' else 1, g)
            steps.append(('spatial', _row(B, rw=vh, rh=vv)))
        elif t == 'translation':
            sh, sw = A.draw_translation(B, H, W, generator=g)
            steps.append(('spatial', _row(B, sh=sh, sw=sw)))
        else:
            r0, r1, c0, c1 = A.draw_cutout(B, H, W, generator=g)
            steps.append(('spatial', _row(B, r0=r0, r1=r1, c0=c0, c1=c1)))
    return steps


@pytest.mark.parametrize('types,flip,launches', CHAINS, ids=['+'.join(t) for t, _, _ in CHAINS])
def test_diffaugment_chain_matches_sequential_reference(types, flip, launches, chain_input, gpu_device, monkeypatch,
                                                        record_testsuite_property):
    """DiffAugment(x, types) == its augmentations applied one after the other by the oracle with the same draws: the row
    merge of _spatial_run and the flush rule.  Spatial-only chains bit-equal, value and gradient; chains with colour
    within 2e-6 / 1e-5 (the gradient through the whole chain)."""
    from histogan_amd import augment as A
    B, C, H, W = CHAIN_SHAPE
    assert W > 128 and H * W > 256 and C * H * W // 4 > 31 * 1024
    x, go, fl = chain_input
    fl = fl if flip else None
    if flip:
        assert 0 < int(fl.sum()) < B       # both values occur
    seed = 100 + len(types) + 10 * launches
    calls, spatial = [], A.augment_spatial
    monkeypatch.setattr(A, 'augment_spatial', lambda t, p: (calls.append(1), spatial(t, p))[1])
    xg = x.to(gpu_device).requires_grad_(True)
    y = A.DiffAugment(xg, types, flip=fl, generator=torch.Generator().manual_seed(seed))
    gx, = torch.autograd.grad(y, xg, go.to(gpu_device))
    assert len(calls) == launches

    xd = x.double().requires_grad_(True)
    yd = xd
    for kind, rows in _redraw(types, fl, B, H, W, torch.Generator().manual_seed(seed)):
        yd = O.spatial(yd, rows) if kind == 'spatial' else O.color(yd, rows.double())
    gd, = torch.autograd.grad(yd, xd, go.double())
    y, gx, yd = y.detach().cpu(), gx.cpu(), yd.detach()
    e = dict(fwd=relmax(y.numpy(), yd.numpy()), adj=relmax(gx.numpy(), gd.numpy()))
    _record(record_testsuite_property, f'augment_shapes/chain/{"+".join(types)}', e)
    assert 0.0 < float((y != x).float().mean())          # the draws did something
    if 'color' in types:
        assert e['fwd'] <= E_FWD and e['adj'] <= E_ADJ, e
    else:
        assert torch.equal(y, yd.float()) and torch.equal(gx, gd.float()), e


# ---- d. second order: the gradient penalty through the augmented real images --------------------------------------------
W_SCALE = 0.05


def _penalty(x, aug, w):
    """The gradient penalty's pattern with f(y) = sum(y^3 w): the gradient of f(aug(x)) is differentiated again."""
    f = (aug(x).pow(3) * w).sum((1, 2, 3))
    gr, = torch.autograd.grad(f, x, torch.ones_like(f), create_graph=True)
    pen = ((gr.flatten(1).norm(dim=1) - 1) ** 2).mean()
    return pen.detach(), torch.autograd.grad(pen, x)[0]


def test_gradient_penalty_through_augmentation(gpu_device, record_testsuite_property):
    """translation -> cutout -> color on (3, 3, 67, 131), value 1e-5 relative and gradient 2e-5 relmax against the same
    expression over the fp64 oracle chain (the bars of test_conv2d_double_backward).

    Scale of w: with w = 0.05 randn the per-sample gradient norms are ~13 (penalty 152), far from the 1 they are compared
    with, so the penalty does not cancel.  The same expression evaluated with torch ops in fp32 on the CPU (the kernels'
    formulas on the float32 inputs) differs from the fp64 one by 3.5e-7 relative in the value and 3.5e-7 relmax in the
    gradient: 1/28 and 1/57 of the bars."""
    from histogan_amd.augment import augment_color, augment_spatial
    B, C, H, W = 3, 3, 67, 131
    assert W > 128 and H % 4 != 0 and (C * H * W) % 4 != 0 and _chunks(C * H * W) > 1
    g = _gen(B, C, H, W, 4)
    x = torch.rand(B, C, H, W, generator=g)
    w = torch.randn(B, C, H, W, generator=g) * W_SCALE
    tr = _row(B, sh=[5, -8, 0], sw=[-9, 16, 3])
    cut = _row(B, r0=[10, 0, 40], r1=[43, 20, 66], c0=[30, 100, 0], c1=[95, 130, 64])
    fused = tr.clone()
    fused[:, 5:9] = cut[:, 5:9]
    col = torch.tensor([[0.3, 1.6, 0.7], [-0.4, 0.3, 1.4], [0.1, 1.0, 1.2]])

    xg = x.to(gpu_device).requires_grad_(True)
    pen, gp = _penalty(xg, lambda t: augment_color(augment_spatial(t, fused), col), w.to(gpu_device))
    xd = x.double().requires_grad_(True)
    pen_d, gp_d = _penalty(xd, lambda t: O.color(O.spatial(O.spatial(t, tr), cut), col.double()), w.double())
    e = dict(value=abs(float(pen) - float(pen_d)) / abs(float(pen_d)), grad=relmax(gp.cpu().numpy(), gp_d.numpy()),
             pen=float(pen_d))
    _record(record_testsuite_property, 'augment_shapes/second_order', e)
    assert float(pen_d) > 1.0 and float(gp_d.abs().max()) > 0
    assert e['value'] <= 1e-5, e
    assert e['grad'] <= 2e-5, e


# ---- e. refusals surface as exceptions -------------------------------------------------------------------------------------
def test_refusals(gpu_device):
    """B C > 65535 (the z extent of the spatial grid) is HG_EINVAL before any launch and raises through check; a
    workspace one byte short is HG_EWORKSPACE."""
    from histogan_amd import augment as A
    from histogan_amd._lib import HgError, lib, stream_of
    B = 21846
    assert B * 3 > 65535
    x = torch.zeros(B, 3, 1, 1, device=gpu_device)
    with pytest.raises(HgError, match='hg_augment_spatial'):
        A.augment_spatial(x, _row(B))
    assert torch.equal(A.augment_spatial(x[:21845], _row(21845)), x[:21845])        # 65535 planes are served

    x = torch.rand(5, 3, 8, 8, device=gpu_device)
    n = lib.hg_augment_workspace_bytes(5)
    assert n > 1
    ws = torch.empty(n, dtype=torch.uint8, device=gpu_device)
    mean = torch.full((5,), -7.0, device=gpu_device)
    rc = lib.hg_sample_mean(x.data_ptr(), mean.data_ptr(), 5, 3 * 8 * 8, ws.data_ptr(), n - 1, stream_of(x))
    assert rc == -4                                                              # HG_EWORKSPACE (include/hg_hist.h)
    assert torch.equal(mean, torch.full_like(mean, -7.0))                        # and nothing ran
    assert lib.hg_sample_mean(x.data_ptr(), mean.data_ptr(), 5, 3 * 8 * 8, ws.data_ptr(), n, stream_of(x)) == 0
    assert relmax(mean.cpu().numpy(), x.double().mean((1, 2, 3)).cpu().numpy()) <= E_MEAN
