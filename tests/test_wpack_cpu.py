"""Host logic of histogan_amd/wpack.py without a GPU: what the batched pack decides for a weight (plan_weights) and the
writable flat gradient slot of a weight (grad_slot).  The expected plans below are written out from the rule, not computed:
a 3x3 weight gets Winograd operands unless (wants_direct and not wants_wino); its direct pack is left lazy when it has both
Winograd operands and not wants_direct; sum_taps W^2 is written by the direct item, or by the Winograd item of a lazy weight."""
import gc

import pytest
import torch

SHAPES = [(40, 24, 3, 3), (3, 70, 1, 1), (130, 33, 3, 3), (64, 64, 3, 3)]
# Winograd operands exist for the 3x3 weights whose reduction side is a multiple of 8 (hg_wino_packed_elems): 24 / 40 and 64 / 64
# channels; not for 1x1, not for 33 / 130 channels.
WINO_CAPABLE = [True, False, False, True]

# per weight: (direct item, Winograd forward operand, Winograd data-gradient operand, writer of wsq)
LAZY = (False, True, True, 'wino')
DIRECT = (True, False, False, 'direct')
BOTH = (True, True, True, 'direct')
EXPECT = {                    # (wants_direct, wants_wino, WINO) set on every weight -> the four weights in order
    'nothing asked': ((False, False, True), [LAZY, DIRECT, DIRECT, LAZY]),
    'wino only': ((False, True, True), [LAZY, DIRECT, DIRECT, LAZY]),
    'direct only': ((True, False, True), [DIRECT, DIRECT, DIRECT, DIRECT]),
    'both': ((True, True, True), [BOTH, DIRECT, DIRECT, BOTH]),
    'WINO off': ((False, True, False), [DIRECT, DIRECT, DIRECT, DIRECT]),
    'WINO off, both': ((True, True, False), [DIRECT, DIRECT, DIRECT, DIRECT]),
}


@pytest.fixture
def records():
    from histogan_amd import wpack as W
    W.enable_pack_cache(None)
    flat = torch.zeros(sum(a * b * c * d for a, b, c, d in SHAPES))
    ps, off = [], 0
    for s in SHAPES:
        n = s[0] * s[1] * s[2] * s[3]
        ps.append(torch.nn.Parameter(flat[off:off + n].view(s)))
        off += n
    W.enable_pack_cache(ps)
    recs = [W.record(p) for p in ps]
    assert len({id(r.owner) for r in recs}) == 1 and recs[0].owner.id == flat.untyped_storage().data_ptr()
    yield recs, ps
    W.enable_pack_cache(None)


def _decisions(sig):
    return [(it.block is not None, it.nf > 0, it.nd > 0, it.wsq) for it in sig]


def _plan(recs, direct, wino, switch):
    from histogan_amd import wpack as W
    for r in recs:
        r.wants_direct, r.wants_wino = direct, wino
    return W.plan_weights(recs, switch)


@pytest.mark.parametrize('case', list(EXPECT))
def test_plan_decisions_offsets_and_wsq_writer(case, records):
    from histogan_amd import wpack as W
    from histogan_amd._lib import lib
    recs, _ = records
    (direct, wino, switch), want = EXPECT[case]
    sig, blocks, wblocks = _plan(recs, direct, wino, switch)
    assert [it.key for it in sig] == [r.key for r in recs]
    assert _decisions(sig) == want
    b = wb = 0
    for it, (Co, Ci, k, _), (has_direct, uf, ud, wsq), capable in zip(sig, SHAPES, want, WINO_CAPABLE):
        assert (uf or ud) <= capable
        # exactly one writer of wsq: the direct item when there is one, else the Winograd item -- which then has to exist
        assert wsq == ('direct' if has_direct else 'wino') and (has_direct or it.wblock is not None)
        assert it.block == (b if has_direct else None) and it.wblock == (wb if uf or ud else None)
        assert it.nf == (lib.hg_wino_packed_elems(Co, Ci, W.PACK_FWD) if uf else 0)
        assert it.nd == (lib.hg_wino_packed_elems(Co, Ci, W.PACK_DGRAD) if ud else 0)
        b += lib.hg_conv_pack_blocks(Co, Ci) if has_direct else 0
        wb += lib.hg_wino_pack_blocks(Co, Ci, int(uf), int(ud)) if uf or ud else 0
    assert (blocks, wblocks) == (b, wb)


def test_plan_signature_changes_exactly_with_a_decision(records):
    recs, _ = records
    sigs = {case: _plan(recs, *flags)[0] for case, (flags, _) in EXPECT.items()}
    for a in EXPECT:
        for b in EXPECT:
            assert (sigs[a] == sigs[b]) == (EXPECT[a][1] == EXPECT[b][1]), (a, b)
    # a flag that decides nothing (1x1 weight, 3x3 weight without Winograd operands) leaves the signature alone; one weight's
    # decision changes it
    base = _plan(recs, False, False, True)[0]
    recs[1].wants_direct = recs[2].wants_direct = recs[2].wants_wino = True
    from histogan_amd import wpack as W
    assert W.plan_weights(recs, True)[0] == base
    recs[3].wants_direct = True
    mixed = W.plan_weights(recs, True)[0]
    assert mixed != base and _decisions(mixed) == [LAZY, DIRECT, DIRECT, DIRECT]


@pytest.mark.parametrize('order', ['direct first', 'wino first'])
def test_plan_does_not_depend_on_the_order_of_the_launches(order, records, monkeypatch):
    """a weight whose first launch ran at a shape the Winograd kernel refuses and whose next one at a served shape
    -- or the other way round -- wants both operands, whatever buffers its operand had at the time."""
    from histogan_amd import wpack as W
    recs, _ = records
    rec = recs[3]
    monkeypatch.setattr(W, 'wino_supported', lambda B, K, N, H, Wd: H >= 8)
    op = W.Operand(None, W.PACK_FWD, rec.ref, rec)        # (stripped of its Winograd buffer by an earlier plan; not stale)
    shapes = [(2, 64, 64, 4, 4), (2, 64, 64, 8, 8)]
    for B, K, N, H, Wd in (shapes if order == 'direct first' else shapes[::-1]):
        if W.wino_operand(op, B, K, N, H, Wd) is None:
            W.direct_operand(op)
    assert rec.wants_direct and rec.wants_wino
    assert _decisions(W.plan_weights(recs, True)[0]) == [LAZY, DIRECT, DIRECT, BOTH]


def test_grad_slot_lookup():
    from histogan_amd import wpack as W
    from histogan_amd.optim import FlatParams
    ps = [torch.nn.Parameter(torch.randn(4, 3, 3, 3)), torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 4, 1, 1))]
    flat = FlatParams(ps)
    offs = [0, 108, 113]
    with torch.no_grad():
        assert all(W.grad_slot(p) is None for p in ps)              # before zero_grad()
        flat.zero_grad()
        assert W.grad_slot(ps[1]) is None                           # 1-D: not a convolution weight
    assert W.grad_slot(ps[0]) is None and W.grad_slot(ps[2]) is None    # grad mode on
    with torch.no_grad():
        for i in (0, 2):
            slot, owner, written, index = W.grad_slot(ps[i])
            want = flat.grad[offs[i]:offs[i] + ps[i].numel()].view(ps[i].shape)
            assert owner is flat and not written
            assert slot.data_ptr() == want.data_ptr() and slot.shape == want.shape
        flat.mark_written(index)
        assert index == 2 and flat.written == {2}
        assert W.grad_slot(ps[2])[2] and not W.grad_slot(ps[0])[2]  # "already written" follows the written set
        flat.mark_written(0)
        assert W.grad_slot(ps[0])[2]
        flat.gather()
        assert W.grad_slot(ps[0]) is None and W.grad_slot(ps[2]) is None    # after gather()
        flat.zero_grad()
        assert W.grad_slot(ps[0]) is not None
        del flat, owner
        gc.collect()
        assert W.grad_slot(ps[0]) is None and W.grad_slot(ps[2]) is None    # the FlatParams is gone
