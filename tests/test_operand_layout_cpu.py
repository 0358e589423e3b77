"""The host-side facts tests/test_operand_layout_gpu.py rests on, without a GPU: the helper's layouts are what they claim, a
flat parameter buffer really puts parameters on 4-byte-only addresses, the ReHistoGAN parameter order does so in shipped
configurations, and ops.grouped_linear_supported refuses the weights hg_grouped_linear_* would refuse."""
import pytest
import torch
from torch import nn

import layout_ref as LR


@pytest.mark.parametrize('shape', [(5,), (3, 7), (2, 3, 5, 7), (1,)])
@pytest.mark.parametrize('k', [1, 2, 3])
def test_shifted_has_the_residue_and_the_values(shape, k):
    t = torch.randn(*shape)
    s = LR.shifted(t, k)
    assert s.data_ptr() % 16 == 4 * k and s.is_contiguous() and s.shape == t.shape and torch.equal(s, t)
    p = LR.shifted(torch.arange(18, dtype=torch.int32).reshape(2, 9), k)
    assert p.data_ptr() % 16 == 4 * k and p.dtype == torch.int32 and int(p[1, 8]) == 17


def _read_as_kernel(v):
    """What a kernel given v.data_ptr() and v.shape reads: numel consecutive elements from the view's first element."""
    return torch.as_strided(v, (v.numel(),), (1,)).reshape(v.shape) if v.numel() <= _reach(v) else None


def _reach(v):
    return v.untyped_storage().nbytes() // v.element_size() - v.storage_offset()


def test_layouts_are_equal_views_a_bare_pointer_misreads():
    """Every view equals its tensor and is not contiguous, and reading it as the kernels read an operand (consecutive
    elements from data_ptr) gives other values: a wrapper that drops f32c from one operand cannot pass the bit-equality
    assertions of the GPU module's non-contiguous cases."""
    t = torch.randn(2, 3, 4, 6)
    t[1] = t[0]
    got = dict(LR.layouts(t))
    assert set(got) == {'channels_last', 'every_other_column', 'batch_expanded'}
    for name, v in got.items():
        assert not v.is_contiguous() and v.shape == t.shape and torch.equal(v, t), name
        raw = _read_as_kernel(v)
        assert raw is None or not torch.equal(raw.nan_to_num(nan=-1.0), t), name
    assert 0 in got['batch_expanded'].stride() and got['channels_last'].stride()[1] == 1
    # 2-d operands (styles, demodulation coefficients): transposed storage and the strided columns
    s = torch.randn(3, 5)
    assert {n for n, _ in LR.layouts(s)} == {'channels_last', 'every_other_column'}
    # an extent that makes a view contiguous is left out rather than passed off as a layout
    assert 'channels_last' not in dict(LR.layouts(torch.randn(2, 1, 4, 4)))


@pytest.mark.parametrize('pad', [0, 1, 2, 3, 4])
def test_flat_params_puts_parameters_behind_an_odd_one_off_alignment(pad):
    from histogan_amd.optim import FlatParams
    ps = [nn.Parameter(torch.randn(4, 2, 3, 3)), nn.Parameter(torch.randn(8, 16)), nn.Parameter(torch.randn(3))]
    vals = [p.detach().clone() for p in ps]
    head = [nn.Parameter(torch.zeros(pad))] if pad else []
    flat = FlatParams(head + ps)
    assert flat.data.data_ptr() % 16 == 0
    off = pad
    for p, v in zip(ps, vals):
        assert p.data_ptr() == flat.data.data_ptr() + 4 * off and p.data_ptr() % 16 == (4 * off) % 16
        assert p.grad.data_ptr() == flat.grad.data_ptr() + 4 * off
        assert p.is_contiguous() and torch.equal(p.detach(), v)
        off += p.numel()
    # a slot offset taken in units of 16 bytes instead of elements would land elsewhere for every pad that is no multiple of 4
    assert (ps[0].data_ptr() - flat.data.data_ptr()) // 4 == pad


@pytest.mark.parametrize('size,residue', [(64, 8), (128, 4), (256, 0)])
def test_rehistogan_flat_order_puts_the_recoloring_head_off_alignment(size, residue):
    """retrainer.recoloringGAN builds FlatParams(ED + G + H) in parameter order: every DecoderBlock.conv_out_rgb.bias has 3
    elements and there are log2(size) - 4 decoder blocks, so the first RecoloringGAN parameter (and everything behind it)
    starts 8 bytes off a 16-byte boundary at image size 64, 4 bytes at 128, aligned at 256."""
    from histogan_amd.nets import HistVectorizer
    from histogan_amd.renets import RecoloringEncoderDecoder, RecoloringGAN
    with torch.device('meta'):
        ED = RecoloringEncoderDecoder(size, network_capacity=16, hist=64, latent_dim=512, style_depth=8)
        G = RecoloringGAN(size, 512, 16)
        H = HistVectorizer(64, 512, 8)
    odd = [n for n, p in ED.named_parameters() if p.numel() % 4]
    assert odd and all(n.endswith('conv_out_rgb.bias') for n in odd) and len(odd) == len(ED.decoder_blocks)
    n_ed = sum(p.numel() for p in ED.parameters())
    assert (4 * n_ed) % 16 == residue
    # nothing in G or H moves the residue again: every later parameter shares it
    assert all(p.numel() % 4 == 0 for p in list(G.parameters()) + list(H.parameters()))


class _OnGpu:
    """The two attributes grouped_linear_supported reads of its first input."""
    is_cuda = True

    def __init__(self, B, K):
        self.shape = (B, K)


def test_grouped_linear_supported_refuses_weights_the_kernels_would_refuse():
    from histogan_amd import ops
    x = _OnGpu(8, 64)
    ws = [torch.randn(n, 64) for n in (128, 4, 260)]
    assert all(w.data_ptr() % 16 == 0 for w in ws)
    assert ops.grouped_linear_supported([x], ws)
    for k in (1, 2, 3):
        for i in range(3):
            bad = list(ws)
            bad[i] = LR.shifted(ws[i], k)
            assert torch.equal(bad[i], ws[i]) and not ops.grouped_linear_supported([x], bad), (k, i)
    for name, v in LR.layouts(ws[2]):
        assert not ops.grouped_linear_supported([x], [ws[0], ws[1], v]), name
    assert not ops.grouped_linear_supported([x], [ws[0], ws[1].double(), ws[2]])
    # the conditions it had before stay
    assert not ops.grouped_linear_supported([_OnGpu(65, 64)], ws)
    assert not ops.grouped_linear_supported([_OnGpu(8, 48)], [torch.randn(8, 48)])
    assert not ops.grouped_linear_supported([x], [torch.randn(6, 64)])


def test_realigned_copies_only_what_is_off_alignment():
    from histogan_amd.ops import _realigned
    t = torch.randn(8, 64)
    assert _realigned(t).data_ptr() == t.data_ptr()
    for k in (1, 2, 3):
        s = LR.shifted(t, k)
        r = _realigned(s)
        assert r.data_ptr() % 16 == 0 and r.is_contiguous() and torch.equal(r, t)
    for name, v in LR.layouts(t):
        r = _realigned(v)
        assert r.data_ptr() % 16 == 0 and r.is_contiguous() and torch.equal(r, t), name
    assert _realigned(t.double()).dtype == torch.float32
