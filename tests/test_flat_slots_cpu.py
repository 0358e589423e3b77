"""optim.FlatParams without a GPU: the slot table every user of the layout reads, and the three phases of a step's gradients
(closed / open for direct writes / gathered) as wpack.grad_slot sees them."""
import itertools

import pytest
import torch


def _params():
    return [torch.nn.Parameter(torch.randn(7)), torch.nn.Parameter(torch.randn(40, 8, 3, 3)),
            torch.nn.Parameter(torch.randn(3, 40, 1, 1)), torch.nn.Parameter(torch.randn(11))]


def test_slot_table_is_the_layout():
    from histogan_amd import wpack as W
    from histogan_amd.optim import FlatParams, conv_first
    ps = _params()
    want_data = [p.detach().clone() for p in ps]
    flat = FlatParams(conv_first(ps))
    assert flat.params == [ps[1], ps[2], ps[0], ps[3]]
    assert [s.index for s in flat.slots] == [0, 1, 2, 3]
    assert [s.numel for s in flat.slots] == [p.numel() for p in flat.params]
    assert [s.offset for s in flat.slots] == [0] + list(itertools.accumulate(p.numel() for p in flat.params))[:-1]
    for p, s in zip(flat.params, flat.slots):
        assert s.view.data_ptr() == flat.grad.data_ptr() + 4 * s.offset and s.view.shape == p.shape
        assert p.data_ptr() == flat.data.data_ptr() + 4 * s.offset and p.grad.data_ptr() == s.view.data_ptr()
    assert all(torch.equal(p.detach(), w) for p, w in zip(ps, want_data))
    assert flat.n_conv == 40 * 8 * 9 + 3 * 40 and flat.numel == flat.n_conv + 7 + 11
    flat.zero_grad()
    with torch.no_grad():
        for i in (0, 1):
            a, b = W.grad_slot(flat.params[i]), W.grad_slot(flat.params[i])
            assert a[0] is b[0] and a[0] is flat.slots[i].view and a[1] is flat and a[3] == i
        assert W.grad_slot(ps[0]) is None and W.grad_slot(ps[3]) is None
    # without a gradient buffer: the same offsets, no views, nothing registered for direct writes
    qs = _params()
    bare = FlatParams(conv_first(qs), with_grad=False)
    assert [(s.offset, s.numel, s.view) for s in bare.slots] == [(s.offset, s.numel, None) for s in flat.slots]
    assert bare.n_conv == flat.n_conv and bare.grad is None
    with torch.no_grad():
        assert W.grad_slot(qs[1]) is None


OPS = ('zero_grad', 'mark_written', 'close', 'gather')


def _expected(seq):
    """(phase, answer of wpack.grad_slot) after `seq` on a fresh FlatParams.  The docstrings: a slot is writable between
    zero_grad() and gather() (or close()); `written` says whether it was marked since that zero_grad(); close() leaves
    gather() still to come; gather() before the first zero_grad() has nothing to do.  None: not writable."""
    phase, written = 'gathered', False
    for op in seq:
        if op == 'zero_grad':
            phase, written = 'open', False
        elif op == 'mark_written':
            written = True
        elif op == 'gather':
            phase = 'gathered'
        elif phase == 'open':
            phase = 'closed'
    return phase, (written if phase == 'open' else None)


@pytest.mark.parametrize('prefix', [(), ('zero_grad',)], ids=['fresh', 'after zero_grad'])
@pytest.mark.parametrize('pair', list(itertools.product(OPS, OPS)), ids=lambda p: '-'.join(p))
def test_phase_transitions(prefix, pair):
    from histogan_amd import optim
    from histogan_amd import wpack as W
    names = {'closed': optim.CLOSED, 'open': optim.OPEN, 'gathered': optim.GATHERED}
    assert len(set(names.values())) == 3
    ps = [torch.nn.Parameter(torch.randn(4, 3, 3, 3)), torch.nn.Parameter(torch.randn(5))]
    flat = optim.FlatParams(ps)
    assert flat.phase == optim.GATHERED and flat.generation == 0 and flat.written == set()
    seq = prefix + pair
    for n, op in enumerate(seq, 1):
        gen = flat.generation
        flat.mark_written(0) if op == 'mark_written' else getattr(flat, op)()
        assert flat.generation == gen + (op == 'zero_grad')
        with torch.no_grad():
            got = W.grad_slot(ps[0])
        phase, want = _expected(seq[:n])
        assert flat.phase == names[phase], seq[:n]
        assert (got is None) if want is None else (got is not None and got[2] == want and got[0] is flat.slots[0].view), seq[:n]
        assert flat.conv_region_final() == (want is True)          # (the one 4-d parameter is the whole region)
        if phase == 'gathered' and 'zero_grad' in seq[:n]:
            assert all(p.grad is s.view for p, s in zip(ps, flat.slots))
        elif op == 'zero_grad':
            assert all(p.grad is None for p in ps)


def test_second_gather_launches_nothing(monkeypatch):
    from histogan_amd.optim import FlatParams
    ps = [torch.nn.Parameter(torch.randn(4, 3, 3, 3)), torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(6)),
          torch.nn.Parameter(torch.randn(2, 4, 1, 1))]
    flat = FlatParams(ps)
    calls = []
    for name in ('_foreach_copy_', '_foreach_zero_', '_foreach_add_'):
        real = getattr(torch, name)
        monkeypatch.setattr(torch, name, lambda *a, _n=name, _r=real: (calls.append(_n), _r(*a))[1])
    flat.gather()                                    # before the first zero_grad(): nothing to do
    assert calls == []
    flat.zero_grad()
    flat.mark_written(3)
    ps[1].grad = torch.ones(5)                       # copied; ps[0], ps[2] zeroed; ps[3] written directly and delivered: added
    ps[3].grad = torch.ones(2, 4, 1, 1)
    flat.gather()
    assert calls == ['_foreach_copy_', '_foreach_zero_', '_foreach_add_']
    before = flat.grad.clone()
    flat.gather()
    assert calls == ['_foreach_copy_', '_foreach_zero_', '_foreach_add_'] and torch.equal(flat.grad, before)
