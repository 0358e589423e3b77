"""Weight gradients on their way into optim.FlatParams.grad, every delivery path against fp64.

In a trainer a registered convolution weight's gradient is not returned to autograd: conv._direct_wgrad writes it into the weight's
slot of the flat gradient buffer on a side stream, overwrite or accumulate decided on the host from FlatParams.written;
hg_demod_weight_term and the one-node generator's to-RGB write take the same flag; FlatParams.gather() merges slots written
directly, delivered by autograd, and both.  The kernel parity files call torch.autograd.grad on unregistered weights and see none
of this.  Here Discriminator(32, 2) and Generator(32, 512, network_capacity=2) are re-homed as the trainers do it (FlatParams,
DiffGrad, enable_pack_cache), batch 3, inputs from seeded CPU generators, and after gather() EVERY parameter's slice of flat.grad
is compared with oracle.histogan_nets in fp64 on the run's own LeakyReLU branches (oracle_step.LreluMasks; caps: flips <= 1e-5 of
the elements, flip margin <= 2e-6; tools/flat_grad_seed_check.py checks the seeds against them on the CPU with the oracle alone).
The networks are driven by a fixed upstream gradient, (out * g).sum(): no hinge, so no extra kink decides a case.

Poison: flat.grad is filled with NaN before every zero_grad() -- zero_grad() does not clear the buffer, so the first write of a step
must overwrite, a parameter without a gradient must become zero, and nothing of the last step may survive.

Every scenario also asserts the path taken (FlatParams.written, the flag conv.grad_slot handed out per write, gather()'s `both`
add, the slice count) and runs a control with direct writes shut off (zero_grad(); close(): autograd delivers everything).

Bar: relmax <= 2e-5 per parameter, the fp64 gradient bar of these small networks (tests/test_gstage_gpu.py,
test_generator_forward_behind_any_pad, test_conv2d_double_backward).  Measured figures: DESIGN.md, beside the flat-buffer section.
"""
import contextlib
import copy
import json

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import relmax

import flat_grad_ref as R

pytestmark = pytest.mark.gpu

BAR = 2e-5


# ---- the run under test -------------------------------------------------------------------------------------------------
def _rehome(module, front=(), back=()):
    """The module's parameters re-homed as the trainers do it; `front` / `back`: further parameters of the same flat buffer."""
    from histogan_amd.conv import enable_pack_cache
    from histogan_amd.optim import DiffGrad, FlatParams
    flat = FlatParams(list(front) + list(module.parameters()) + list(back))
    enable_pack_cache(list(module.parameters()) + [p for p in list(front) + list(back) if p.dim() == 4])
    return flat, DiffGrad(flat, lr=2e-4, betas=(0.5, 0.9))


def _open(flat, direct=True):
    """A new generation over a poisoned buffer; direct=False: the control, every gradient goes through autograd."""
    flat.grad.fill_(float('nan'))
    flat.zero_grad()
    if not direct:
        flat.close()
        assert flat.slot(0) is None


def _conv_slots(flat):
    return {s.index for p, s in zip(flat.params, flat.slots) if p.dim() == 4}


def _gathered(flat, named, grad_mode=True):
    """gather(), then {name: the parameter's slice of flat.grad}: finite, and p.grad IS the slot."""
    index = {id(p): i for i, p in enumerate(flat.params)}
    with torch.set_grad_enabled(grad_mode):
        flat.gather()
    torch.cuda.synchronize()
    out = {}
    for n, p in named:
        s = flat.slots[index[id(p)]]
        assert p.grad is s.view and s.view.data_ptr() == flat.grad.data_ptr() + 4 * s.offset, n
        assert p.data_ptr() == flat.data.data_ptr() + 4 * s.offset and s.numel == p.numel(), n
        g = flat.grad[s.offset:s.offset + s.numel].view(p.shape).detach().clone()
        assert bool(torch.isfinite(g).all()), 'poison left in ' + n
        out[n] = g
    return out


@contextlib.contextmanager
def _branches():
    """The LeakyReLU branches (out > 0) of every feature map the networks produce inside, in forward order."""
    from histogan_amd import gfused, nets, ops
    masks = []

    def rec(orig):
        def f(*a, **k):
            out = orig(*a, **k)
            masks.append(out.detach().cpu() > 0)
            return out
        return f

    saved = nets.conv2d_lrelu, ops.demod_noise_lrelu, ops.conv_dnl
    nets.conv2d_lrelu, ops.demod_noise_lrelu, ops.conv_dnl = (rec(f) for f in saved)
    gfused.STAGE_OBSERVER = lambda out: masks.append(out.detach().cpu() > 0)
    try:
        yield masks
    finally:
        nets.conv2d_lrelu, ops.demod_noise_lrelu, ops.conv_dnl = saved
        gfused.STAGE_OBSERVER = None


class _SlotSpy:
    """conv.grad_slot with a log: per query (slot index, the `already written` flag handed out), or None where it answered None."""

    def __init__(self, monkeypatch):
        from histogan_amd import conv
        self.log, orig = [], conv.grad_slot

        def spy(w):
            ws = orig(w)
            self.log.append(None if ws is None else (ws[3], ws[2]))
            return ws

        monkeypatch.setattr(conv, 'grad_slot', spy)

    def take(self):
        log, self.log[:] = list(self.log), []
        return log

    @staticmethod
    def flags(log):
        out = {}
        for i, written in (e for e in log if e is not None):
            out.setdefault(i, []).append(written)
        return out


@pytest.fixture
def spy(monkeypatch):
    return _SlotSpy(monkeypatch)


@pytest.fixture(scope='module')
def d0():
    return R.discriminator()


@pytest.fixture(scope='module')
def g0():
    return R.generator()


def _d_loss(D, p, dev):
    """(D(x) * gl).sum() [+ trainer.gradient_penalty] -> (loss, the pass's branches)."""
    from histogan_amd.trainer import gradient_penalty
    x = p['x'].to(dev).requires_grad_(p['penalty'])
    with _branches() as masks:
        out, _ = D(x)
    loss = (out * p['gl'].to(dev)).sum()
    if p['penalty']:
        loss = loss + gradient_penalty(x, out)
    return loss, masks


def _run_d(d0, dev, passes, scales, direct, joint=False, after_pass=None, create_graph=(), front=(), back=(), frozen=(), warm=None,
           before=None):
    """One generation of the re-homed discriminator over `passes`: one backward per pass (joint: ONE backward of the sum).
    warm: a pass run through a whole earlier generation (gradients of another step in the buffer before the poison).
    before: called once the generation is open.  -> ([(name, parameter)] for _gathered, [branches per pass], flat), gather() not
    yet called."""
    D = copy.deepcopy(d0).to(dev)
    for n, p in D.named_parameters():
        if frozen and n.startswith(tuple(frozen)):
            p.requires_grad_(False)
    flat, opt = _rehome(D, front, back)
    D.train()
    if warm is not None:
        flat.zero_grad()
        _d_loss(D, warm, dev)[0].backward()
        flat.gather()
    _open(flat, direct)
    if before is not None:
        before()
    masks, total = [], 0.0
    for i, (p, s) in enumerate(zip(passes, scales)):
        loss, m = _d_loss(D, p, dev)
        masks.append(m)
        if joint:
            total = total + loss * s
        else:
            (loss * s).backward(create_graph=i in create_graph)
        if after_pass is not None:
            after_pass(i, flat)
    if joint:
        total.backward()
    named = list(D.named_parameters()) + [('front%d' % i, p) for i, p in enumerate(front)] + [('back%d' % i, p) for i, p in enumerate(back)]
    return named, masks, flat


def _same_masks(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(torch.equal(u, v) for u, v in zip(x, y)) for x, y in zip(a, b))


def _report(record_testsuite_property, name, got, want, tol=BAR):
    """Every parameter's slice against fp64: print and record the worst, assert the bar; a gradient that is zero in fp64 is zero."""
    n, e, errs = R.worst(got, want)
    print('flat_grad_paths %s: worst %s relmax %.2e (bar %.0e)' % (name, n, e, tol))
    record_testsuite_property('flat_grad_paths/' + name, json.dumps(dict(worst=n, relmax=e, bar=tol)))
    for k, w in want.items():
        assert got[k].shape == w.shape, k
        if not bool(w.any()):
            assert not bool(got[k].any()), 'a gradient no loss reaches is not zero: ' + k
    bad = {k: v for k, v in errs.items() if not v <= tol}
    assert not bad, (name, bad)


# ---- discriminator --------------------------------------------------------------------------------------------------------
def test_discriminator_plain_backward(d0, gpu_device, spy, record_testsuite_property):
    """1.  One plain backward: every convolution weight is written directly, once, as an overwrite; the control through autograd
    gives the same bits (one contribution per weight, deterministic kernels).  Ties
    test_discriminator_is_the_same_bits_behind_any_pad (pad 0) to fp64."""
    passes, scales = R.d_scenario('plain')
    named, masks, flat = _run_d(d0, gpu_device, passes, scales, True)
    conv = _conv_slots(flat)
    assert flat.written == conv and len(conv) == 19
    assert _SlotSpy.flags(spy.take()) == {i: [False] for i in conv}
    assert all(p.grad is None for p in flat.params if p.dim() == 4)
    got = _gathered(flat, named)
    _report(record_testsuite_property, 'd_plain', got, R.d_truth(d0, passes, masks, scales))

    named, masks_c, flat = _run_d(d0, gpu_device, passes, scales, False)
    assert flat.written == set() and all(e is None for e in spy.take())
    ctl = _gathered(flat, named)
    assert _same_masks(masks, masks_c)
    assert [k for k in got if not torch.equal(got[k], ctl[k])] == []


def test_discriminator_two_passes_in_one_generation(d0, gpu_device, spy, record_testsuite_property):
    """2.  A fake-like and a real-like pass between one zero_grad() and one gather(): the second pass finds every slot written
    and accumulates.  fp64: the gradient of the sum."""
    passes, scales = R.d_scenario('two_passes')
    seen = []

    def after(i, flat):
        seen.append((set(flat.written), _SlotSpy.flags(spy.take())))

    named, masks, flat = _run_d(d0, gpu_device, passes, scales, True, after_pass=after)
    conv = _conv_slots(flat)
    assert seen[0] == (conv, {i: [False] for i in conv}), 'first pass: every slot written once, as an overwrite'
    assert seen[1] == (conv, {i: [True] for i in conv}), 'second pass: every write accumulates'
    truth = R.d_truth(d0, passes, masks, scales)
    _report(record_testsuite_property, 'd_two_passes', _gathered(flat, named), truth)

    named, masks_c, flat = _run_d(d0, gpu_device, passes, scales, False)
    assert flat.written == set() and all(e is None for e in spy.take()) and _same_masks(masks, masks_c)
    _report(record_testsuite_property, 'd_two_passes/autograd', _gathered(flat, named), truth)


def test_discriminator_gradient_penalty_step(d0, gpu_device, spy, record_testsuite_property):
    """3.  The D phase of a gradient-penalty step as trainer.discriminator_phase(two_passes=True) + trainer.gradient_penalty build
    it: D(fake), D(real), ONE plain backward of divergence-like term + penalty.  Per weight the fake pass's first-order term, the
    real pass's, and the penalty's second-order term (through _ConvDgrad.backward) land in one slot: one overwrite, then
    accumulates.  fp64: the double backward of the oracle."""
    passes, scales = R.d_scenario('penalty')
    named, masks, flat = _run_d(d0, gpu_device, passes, scales, True, joint=True)
    conv = _conv_slots(flat)
    flags = _SlotSpy.flags(spy.take())
    assert flat.written == conv and set(flags) == conv
    assert all(f == [False] + [True] * (len(f) - 1) and len(f) >= 3 for f in flags.values()), flags
    truth = R.d_truth(d0, passes, masks, scales)
    _report(record_testsuite_property, 'd_penalty', _gathered(flat, named), truth)

    named, masks_c, flat = _run_d(d0, gpu_device, passes, scales, False, joint=True)
    assert flat.written == set() and all(e is None for e in spy.take()) and _same_masks(masks, masks_c)
    _report(record_testsuite_property, 'd_penalty/autograd', _gathered(flat, named), truth)


def test_discriminator_gradient_accumulation(d0, gpu_device, spy, record_testsuite_property):
    """4.  Three micro-batches, loss / 3, between one zero_grad() and one gather().  fp64: the gradient of the mean."""
    passes, scales = R.d_scenario('accumulation')
    seen = []
    named, masks, flat = _run_d(d0, gpu_device, passes, scales, True, after_pass=lambda i, f: seen.append(_SlotSpy.flags(spy.take())))
    conv = _conv_slots(flat)
    assert flat.written == conv
    assert seen == [{i: [False] for i in conv}] + [{i: [True] for i in conv}] * 2
    truth = R.d_truth(d0, passes, masks, scales)
    _report(record_testsuite_property, 'd_accumulation', _gathered(flat, named), truth)

    named, masks_c, flat = _run_d(d0, gpu_device, passes, scales, False)
    assert flat.written == set() and all(e is None for e in spy.take()) and _same_masks(masks, masks_c)
    _report(record_testsuite_property, 'd_accumulation/autograd', _gathered(flat, named), truth)


@pytest.mark.parametrize('graph_pass', [0, 1], ids=['graph_first', 'plain_first'])
def test_both_routes_in_one_step(graph_pass, d0, gpu_device, spy, monkeypatch, record_testsuite_property):
    """5.  One contribution from a backward with create_graph=True (grad mode on: no direct write, autograd delivers), one from a
    plain backward (written directly), in either order: gather() adds autograd's part onto the written slot (`both`)."""
    passes, scales = R.d_scenario('both_routes')
    seen = []
    named, masks, flat = _run_d(d0, gpu_device, passes, scales, True, create_graph=(graph_pass,),
                                after_pass=lambda i, f: seen.append((set(f.written), spy.take())))
    conv = _conv_slots(flat)
    written, log = seen[graph_pass]
    assert all(e is None for e in log) and len(log) >= len(conv), 'the recorded pass wrote nothing directly'
    assert written == (set() if graph_pass == 0 else conv)
    assert seen[1 - graph_pass][0] == conv and _SlotSpy.flags(seen[1 - graph_pass][1]) == {i: [False] for i in conv}
    slots = {i: flat.slots[i].view for i in conv}
    assert all(flat.params[i].grad is not None and flat.params[i].grad.data_ptr() != slots[i].data_ptr() for i in conv)
    adds, orig = [], torch._foreach_add_

    def counting(dst, src, *a, **k):
        adds.append([d.data_ptr() for d in dst])
        return orig(dst, src, *a, **k)

    monkeypatch.setattr(torch, '_foreach_add_', counting)
    got = _gathered(flat, named, grad_mode=False)      # (the recorded pass left gradients that carry a graph: keep it out of flat.grad)
    monkeypatch.setattr(torch, '_foreach_add_', orig)
    assert len(adds) == 1 and sorted(adds[0]) == sorted(v.data_ptr() for v in slots.values()), 'gather() did not take its `both` branch'
    _report(record_testsuite_property, 'd_both_routes/' + ('graph_first', 'plain_first')[graph_pass], got,
            R.d_truth(d0, passes, masks, scales))


def test_parameters_no_loss_reaches_become_zero(d0, gpu_device, spy, record_testsuite_property):
    """6.  A frozen block, an unused convolution weight in front of the network (everything behind it 8 bytes off a 16-byte
    boundary) and an unused vector behind it, after a whole earlier step and the poison: their slices are zeros, nothing of the
    earlier step is left anywhere, and the rest equals fp64."""
    dev = gpu_device
    passes, scales = R.d_scenario('unreached')
    front = [nn.Parameter(torch.ones(2, 3, 3, 3, device=dev))]
    back = [nn.Parameter(torch.ones(5, device=dev))]
    named, masks, flat = _run_d(d0, dev, passes[1:], scales[1:], True, front=front, back=back, frozen=('blocks.1.',), warm=passes[0],
                                before=spy.take)
    frozen = {i for i, p in enumerate(flat.params) if not p.requires_grad}
    conv = _conv_slots(flat)
    assert len(frozen) == 8 and 0 in conv and flat.slots[1].offset == 54
    assert flat.written == conv - frozen - {0}
    assert _SlotSpy.flags(spy.take()) == {i: [False] for i in flat.written}
    got = _gathered(flat, named)
    for n in ['front0', 'back0'] + [n for n in got if n.startswith('blocks.1.')]:
        assert not bool(got.pop(n).any()), n
    truth = R.d_truth(d0, passes[1:], masks, scales[1:], frozen=('blocks.1.',))
    _report(record_testsuite_property, 'd_unreached', got, {n: t for n, t in truth.items() if n in got})


# ---- generator ------------------------------------------------------------------------------------------------------------
def _g_forward(G, mode, t, noise):
    from histogan_amd import gfused
    from histogan_amd.nets import _noise_t
    if mode == 'one_node':
        nzt = _noise_t(noise)
        assert gfused.supported(G, t, nzt)
        return gfused.generator_train(G, t, nzt)
    x, rgb = G.initial_block.expand(noise.shape[0], -1, -1, -1), None
    for i, blk in enumerate(G.blocks):
        x, rgb = blk.forward_(x, rgb, t[3 * i], t[3 * i + 1], t[3 * i + 2], inoise=noise)
    return rgb


def _run_g(g0, dev, mode, passes, direct, after_pass=None):
    G = copy.deepcopy(g0).to(dev)
    flat, opt = _rehome(G)
    G.train()
    _open(flat, direct)
    masks, gts, imgs = [], [], []
    for i, p in enumerate(passes):
        t = [u.to(dev).requires_grad_(True) for u in p['t']]
        with _branches() as m:
            rgb = _g_forward(G, mode, t, p['noise'].to(dev))
        assert len(m) == 2 * len(G.blocks)
        rgb.backward(p['gout'].to(dev))
        masks.append(m)
        gts.append([u.grad.detach().clone() for u in t])
        imgs.append(rgb.detach().clone())
        if after_pass is not None:
            after_pass(i, flat)
    return list(G.named_parameters()), masks, flat, gts, imgs


@pytest.mark.parametrize('mode', ['one_node', 'per_block'])
def test_generator_two_backward_passes_in_one_generation(mode, g0, gpu_device, spy, record_testsuite_property):
    """7.  Two forward / backward passes of the generator (projected styles as inputs, as in
    test_generator_stages_are_the_same_bits_behind_any_pad) in one generation.  First pass: conv._direct_wgrad overwrites,
    hg_demod_weight_term adds behind it, the one-node pass writes the to-RGB slots.  Second pass: both accumulate; the one-node
    pass finds its to-RGB slots taken and hands that gradient to autograd, which gather() adds (`both`).  fp64: the sum; the
    to_style layers, which no loss reaches here, get zeros."""
    dev = gpu_device
    passes = R.g_scenario(g0)
    seen = []
    named, masks, flat, gts, imgs = _run_g(g0, dev, mode, passes, True,
                                           after_pass=lambda i, f: seen.append((set(f.written), _SlotSpy.flags(spy.take()))))
    conv = _conv_slots(flat)
    index = {id(p): i for i, p in enumerate(flat.params)}
    rgb = {index[id(p)] for n, p in named if n.endswith('to_rgb.conv.weight')}
    assert len(conv) == 12 and len(rgb) == 4 and rgb < conv
    direct = conv if mode == 'one_node' else conv - rgb
    assert seen[0][0] == direct and seen[1][0] == direct
    # per modulated convolution: the weight gradient and the demodulation term, in this order; the to-RGB slot: one query
    want = lambda first: {i: ([first] if i in rgb else [first, True]) for i in direct}
    assert seen[0][1] == want(False) and seen[1][1] == want(True), seen
    both = {i for i in flat.written if flat.params[i].grad is not None}
    assert both == (rgb if mode == 'one_node' else set())
    got = _gathered(flat, named)
    truth, gt64, img64 = R.g_truth(g0, passes, masks)
    for k in range(2):
        assert relmax(imgs[k].cpu().numpy(), img64[k].numpy()) <= 1e-6
        e = max(R.relmax_t(a, b) for a, b in zip(gts[k], gt64[k]))
        assert e <= BAR, ('projected styles, pass %d' % k, e)
    _report(record_testsuite_property, 'g_two_passes/' + mode, got, truth)

    named, masks_c, flat, gts_c, imgs_c = _run_g(g0, dev, mode, passes, False)
    assert flat.written == set() and all(e is None for e in spy.take()) and _same_masks(masks, masks_c)
    assert all(torch.equal(a, b) for a, b in zip(imgs, imgs_c))
    _report(record_testsuite_property, 'g_two_passes/%s/autograd' % mode, _gathered(flat, named), truth)


# ---- batch slicing at toy sizes -------------------------------------------------------------------------------------------
SLICE_B, SLICE_K, SLICE_N, SLICE_H = 5, 6, 10, 8
SLICED = ['conv2d_k1', 'conv2d_k3', 'conv2d_s2', 'conv2d_lrelu', 'conv2d_same', 'conv2d_add']


def _slice_case(name):
    """-> (call(x, w, b, addend), fp64 reference of the same, kernel size, stride)."""
    from histogan_amd import conv as C
    k, stride = (1 if name == 'conv2d_k1' else 3), (2 if name == 'conv2d_s2' else 1)
    ref = lambda x, w, b, a: F.conv2d(x, w, b, stride=stride, padding=k // 2)
    if name == 'conv2d_lrelu':
        return (lambda x, w, b, a: C.conv2d_lrelu(x, w, b, 0.2)), (lambda x, w, b, a: F.leaky_relu(ref(x, w, b, a), 0.2)), k, stride
    if name == 'conv2d_same':
        return (lambda x, w, b, a: C.conv2d_same(x, w, b)), ref, k, stride
    if name == 'conv2d_add':
        return (lambda x, w, b, a: C.conv2d_add(x, w, b, a)), (lambda x, w, b, a: ref(x, w, b, a) + a), k, stride
    return (lambda x, w, b, a: C.conv2d(x, w, b, stride)), ref, k, stride


def _slice_operands(name, k, stride, dev):
    g = R.cpu_gen('slice', name)
    B, K, N, H = SLICE_B, SLICE_K, SLICE_N, SLICE_H
    Ho = (H - 1) // stride + 1
    x = torch.randn(B, K, H, H, generator=g)
    w = torch.randn(N, K, k, k, generator=g) / (K * k * k) ** 0.5
    b, a, go = torch.randn(N, generator=g), torch.randn(B, N, Ho, Ho, generator=g), torch.randn(B, N, Ho, Ho, generator=g)
    per = max(K * H * H, N * Ho * Ho)
    return [t.to(dev) for t in (x, w, b, a)], go.to(dev), per


class _Pieces:
    """conv._batch_pieces with a log of what it answered."""

    def __init__(self, monkeypatch):
        from histogan_amd import conv
        self.log, orig = [], conv._batch_pieces

        def spy(x, w, stride):
            n = orig(x, w, stride)
            self.log.append((x.shape[0], n))
            return n

        monkeypatch.setattr(conv, '_batch_pieces', spy)


@pytest.mark.parametrize('name', SLICED)
def test_batch_slices_match_fp64_and_the_unsliced_call(name, gpu_device, monkeypatch, record_testsuite_property):
    """conv._I32 set to two samples' worth of elements: five images run as slices of 2, 2 and 1 (conv2d_add: its fallback,
    conv2d(...) + addend).  Output, data, weight and bias gradient (conv2d_add: the addend's as well) against F.conv2d in fp64 at
    the bars of tests/test_conv_gpu.py, and against the unsliced call on the same data at the same bars."""
    from histogan_amd import conv as C
    call, ref, k, stride = _slice_case(name)
    ops, go, per = _slice_operands(name, k, stride, gpu_device)
    bars = [2e-6, 2e-6, 5e-6, 5e-6, 2e-6]

    def run():
        leaves = [t.clone().requires_grad_(True) for t in ops]
        out = call(*leaves)
        return [out.detach()] + list(torch.autograd.grad(out, leaves, go, allow_unused=True))

    pieces = _Pieces(monkeypatch)
    monkeypatch.setattr(C, '_I32', 2 * per)
    sliced = run()
    assert (SLICE_B, 3) in pieces.log, pieces.log
    monkeypatch.setattr(C, '_I32', 2 ** 31 - 1)
    del pieces.log[:]
    whole = run()
    assert all(n == 1 for _, n in pieces.log) and pieces.log
    l64 = [t.double().cpu().requires_grad_(True) for t in ops]
    o64 = ref(*l64)
    t64 = [o64.detach()] + list(torch.autograd.grad(o64, l64, go.double().cpu(), allow_unused=True))
    used = range(5) if name == 'conv2d_add' else (0, 1, 2, 3)
    what = ['out', 'gx', 'gw', 'gb', 'gaddend']
    fig = {}
    for i in used:
        es, ew, ex = (relmax(a.cpu().numpy(), b.cpu().numpy()) for a, b in ((sliced[i], t64[i]), (whole[i], t64[i]), (whole[i], sliced[i])))
        print('batch slices %s %s: sliced %.2e unsliced %.2e between %.2e' % (name, what[i], es, ew, ex))
        fig[what[i]] = dict(sliced=es, unsliced=ew, between=ex)
        assert sliced[i].shape == t64[i].shape and es <= bars[i] and ew <= bars[i] and ex <= bars[i], (name, what[i], es, ew, ex)
    record_testsuite_property('flat_grad_paths/slices/' + name, json.dumps(fig))


@pytest.mark.parametrize('stride,k', [(1, 3), (2, 3), (1, 1)])
def test_batch_slices_double_backward(stride, k, gpu_device, monkeypatch):
    """The gradient-penalty pattern of tests/test_conv_gpu.py::test_conv2d_double_backward with both layers sliced, at that
    test's 2e-5."""
    from histogan_amd import conv as C
    from histogan_amd.conv import conv2d, input_grads_only
    g = R.cpu_gen('slice_penalty', stride, k)
    B, K, N, H = SLICE_B, SLICE_K, SLICE_N, SLICE_H
    x = torch.randn(B, K, H, H, generator=g).to(gpu_device).requires_grad_(True)
    w1 = (torch.randn(N, K, k, k, generator=g) / (K * k * k) ** 0.5).to(gpu_device).requires_grad_(True)
    b1 = torch.randn(N, generator=g).to(gpu_device).requires_grad_(True)
    w2 = (torch.randn(4, N, 3, 3, generator=g) / (N * 9) ** 0.5).to(gpu_device).requires_grad_(True)

    def penalty(conv, x, w1, b1, w2, ctx):
        h = F.leaky_relu(conv(x, w1, b1, stride), 0.2)
        out = conv(h, w2, None, 1).pow(2).sum(dim=(1, 2, 3))
        with ctx():
            gr, = torch.autograd.grad(out, x, torch.ones_like(out), create_graph=True)
        return ((gr.reshape(B, -1).norm(2, dim=1) - 1) ** 2).mean()

    Ho = (H - 1) // stride + 1
    pieces = _Pieces(monkeypatch)
    monkeypatch.setattr(C, '_I32', 2 * max(K * H * H, N * Ho * Ho))      # (the second layer: 10 x Ho x Ho per sample, sliced as well)
    ours = penalty(conv2d, x, w1, b1, w2, input_grads_only)
    assert [n > 1 for b, n in pieces.log if b == B] == [True, True], pieces.log
    g_ours = torch.autograd.grad(ours, (x, w1, b1, w2))
    xd, w1d, b1d, w2d = (t.detach().double().cpu().requires_grad_(True) for t in (x, w1, b1, w2))
    ref = penalty(lambda a, w, b, s: F.conv2d(a, w, b, stride=s, padding=w.shape[2] // 2), xd, w1d, b1d, w2d, contextlib.nullcontext)
    g_ref = torch.autograd.grad(ref, (xd, w1d, b1d, w2d))
    assert abs(float(ours.detach()) - float(ref.detach())) <= 1e-5 * max(1.0, abs(float(ref.detach())))
    for n, a, b in zip(('gx', 'gw1', 'gb1', 'gw2'), g_ours, g_ref):
        e = relmax(a.cpu().numpy(), b.numpy())
        print('batch slices penalty s%d k%d %s: %.2e' % (stride, k, n, e))
        assert e <= 2e-5, (n, e)


@pytest.mark.parametrize('name', ['conv2d_k3', 'conv2d_s2', 'conv2d_lrelu', 'conv2d_add'])
def test_batch_slices_into_an_open_flat_slot(name, gpu_device, monkeypatch, spy):
    """A sliced layer whose weight is registered in an open FlatParams: the slices' weight gradients go into the slot one after
    the other (one overwrite, two accumulates); after gather() it holds the fp64 gradient of the WHOLE batch."""
    from histogan_amd import conv as C
    call, ref, k, stride = _slice_case(name)
    (x, w, b, a), go, per = _slice_operands(name, k, stride, gpu_device)
    w, b = nn.Parameter(w), nn.Parameter(b)
    pad = nn.Parameter(torch.zeros(3, device=gpu_device))
    flat, opt = _rehome(nn.ParameterList([w, b]), front=[pad])
    _open(flat)
    pieces = _Pieces(monkeypatch)
    monkeypatch.setattr(C, '_I32', 2 * per)
    call(x, w, b, a).backward(go)
    assert (SLICE_B, 3) in pieces.log and sorted(b for b, n in pieces.log if n == 1) == [1, 2, 2], pieces.log
    assert flat.written == {1} and _SlotSpy.flags(spy.take()) == {1: [False, True, True]}
    got = _gathered(flat, [('pad', pad), ('w', w), ('b', b)])
    l64 = [t.detach().double().cpu().requires_grad_(True) for t in (x, w, b, a)]
    gw, gb = torch.autograd.grad(ref(*l64), l64[1:3], go.double().cpu())
    assert not bool(got['pad'].any())
    for n, t in (('w', gw), ('b', gb)):
        e = R.relmax_t(got[n], t)
        print('batch slices into a flat slot %s g%s: %.2e' % (name, n, e))
        assert e <= 5e-6, (name, n, e)


def test_a_sample_past_the_index_range_is_refused_before_any_launch(gpu_device, monkeypatch):
    """One sample alone above conv._I32: ValueError from every entry point, and nothing was packed or launched."""
    from histogan_amd import conv as C
    launched = []
    for fn in ('pack_weights', 'conv_fwd_packed', 'conv_fwd_add_packed', 'modconv_fwd_packed', 'wino_conv'):
        monkeypatch.setattr(C, fn, lambda *a, _fn=fn, **k: launched.append(_fn))
    for name in SLICED:
        call, ref, k, stride = _slice_case(name)
        ops, go, per = _slice_operands(name, k, stride, gpu_device)
        monkeypatch.setattr(C, '_I32', per - 1)
        with pytest.raises(ValueError, match='exceeds'):
            call(*ops)
        monkeypatch.setattr(C, '_I32', per)            # (exactly at the limit: one image per slice, no error from the check)
        assert C._batch_pieces(ops[0], ops[1], stride) == SLICE_B
    assert launched == []
