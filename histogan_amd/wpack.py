"""Weight-side bookkeeping of the convolutions (conv.py holds the launch wrappers and the autograd Functions).

One registry, keyed by (data_ptr, shape), holds a `_Record` per registered convolution weight: its packed-operand cache
(`enable_pack_cache`) and its slot in the optimizer's flat gradient buffer (`register_grad_slots`).  One `_Owner` per flat buffer
holds what its weights share: generation counter, batched-pack plan, pending pack events.  `pack_weights(w, mode)` returns an
`Operand`; a launch wrapper takes its Winograd buffer (`wino_operand`) or its direct one (`direct_operand`), and these two calls
are also where a registered weight learns which operands its launches want.
"""
import collections
import ctypes
import functools
import os
import weakref

import torch

from ._lib import check, lib, on_device, ptr, raw_stream, stream_of

PACK_FWD, PACK_DGRAD = 0, 1

# Winograd F(2x2, 3x3) for the 3x3 stride-1 output / data-gradient launches (include/hg_wino.h): an operand carries the
# transformed twin of its weight (registered weights: written by the batched pack; others: packed on first use); a launch
# takes it when hg_wino_supported says the shape is served and faster.
WINO = os.environ.get('HG_WINO', '1') != '0'


@functools.lru_cache(maxsize=None)
def wino_supported(B, K, N, H, W):
    return bool(WINO and lib.hg_wino_supported(B, K, N, H, W))


def _wino_pack(w, mode):
    Co, Ci = w.shape[:2]
    n = lib.hg_wino_packed_elems(Co, Ci, mode)
    if not n:
        return False
    with on_device(w.device):
        u = torch.empty(n, dtype=torch.float32, device=w.device)
        check(lib.hg_wino_pack_weights(w.data_ptr(), u.data_ptr(), Co, Ci, mode, stream_of(w)), 'hg_wino_pack_weights')
    return u


def _pack_weights(w, mode):
    Co, Ci, k, _ = w.shape
    n = lib.hg_conv_packed_elems(Co, Ci, k, mode)
    if n == 0:
        raise ValueError(f'conv weights {tuple(w.shape)}: only square 1x1 / 3x3 kernels are implemented')
    with on_device(w.device):
        wt = torch.empty(n, dtype=torch.float32, device=w.device)
        check(lib.hg_conv_pack_weights(w.data_ptr(), wt.data_ptr(), Co, Ci, k, mode, stream_of(w)), 'hg_conv_pack_weights')
    return wt


def _pack_both(w):
    Co, Ci, k, _ = w.shape
    with on_device(w.device):
        wf, wd = (torch.empty(lib.hg_conv_packed_elems(Co, Ci, k, m), dtype=torch.float32, device=w.device) for m in (0, 1))
        check(lib.hg_conv_pack_weights_both(w.data_ptr(), wf.data_ptr(), wd.data_ptr(), Co, Ci, k, stream_of(w)),
              'hg_conv_pack_weights_both')
    return wf, wd


# ---- the registry --------------------------------------------------------------------------------------------------
# Only tensors registered with `enable_pack_cache(params)` are cached: the Trainer registers its convolution weights, which
# live in one flat buffer for the life of the model and only change through DiffGrad.step / ema_update / load_state_dict --
# the first two update through raw pointers (no version counter moves) and therefore call `weights_changed()`.  Everything
# else (plain torch users, the temporaries of a double backward) is packed on every call.
class _Owner:
    """What the registered weights of one flat buffer share.  id: the buffer's base address; gen: bumped when its weights change;
    plan: the batched-pack plan (_Plan)."""
    __slots__ = ('id', 'gen', 'plan', 'events')

    def __init__(self, id):
        self.id, self.gen, self.plan = id, 0, None
        self.events = []      # [[event behind a pack on another stream, ids of the streams that wait for it, keys it covers]]


class _Record:
    """One registered convolution weight.  slot: (weakref to the FlatParams, index in its slot table) of its gradient slot, or None;
    geom: its sizes in the batched pack, asked once (plan_weights)."""
    __slots__ = ('key', 'ref', 'owner', 'slot', 'geom', 'stamp', 'ops', 'vals', 'wants_direct', 'wants_wino')

    def __init__(self, key, p):
        self.key, self.ref, self.slot, self.geom = key, weakref.ref(p), None, None
        self.reset(None)

    def reset(self, owner):
        self.owner = owner    # its flat buffer's _Owner (`.id`: the buffer id); None: not registered for operand caching
        self.stamp = None     # (owner generation, version counter) `ops` and `vals` were made at
        self.ops = None, None # [forward Operand, data-gradient Operand]
        self.vals = {}        # tag -> cached(w, tag, ...) value; 'wsq' comes from the batched pack
        # sticky: a launch took this weight's direct operand / ran at a shape the Winograd kernel serves (plan_weights)
        self.wants_direct = self.wants_wino = False

    def restamp(self, st):
        if self.stamp != st:
            self.stamp, self.ops, self.vals = st, (None, None), {}


_registry = {}       # (data_ptr, shape) -> _Record
_owners = {}         # base address of a flat buffer -> _Owner
_streams = {}        # ('pack' | 'wgrad', device index) -> torch.cuda.Stream


def _device_stream(kind, device):
    key = (kind, device.index)
    return _streams.get(key) or _streams.setdefault(key, torch.cuda.Stream(device=device))


def record(w):
    """The record of a registered, still-alive weight at w's address and shape; None (and a record whose parameter has died
    or moved dropped, so that a later tensor allocated at the same address cannot hit it) otherwise."""
    key = (w.data_ptr(), tuple(w.shape))
    rec = _registry.get(key)
    if rec is None:
        return None
    p = rec.ref()
    if p is None or p.data_ptr() != key[0]:
        del _registry[key]
        return None
    return rec


def _register(p):
    key = (p.data_ptr(), tuple(p.shape))
    return record(p) or _registry.setdefault(key, _Record(key, p))


def enable_pack_cache(params=None):
    """Register convolution weights (4-D tensors among `params`) for packed-weight caching; None switches caching off
    and drops every registration.  Registration is ADDITIVE (a HistoGAN Trainer and a recoloring Trainer built side by
    side -- the reference CLI does that -- both keep their entries) and holds only a weak reference to the parameter."""
    if params is None:
        _owners.clear()
        for key, rec in list(_registry.items()):
            rec.reset(None)
            if rec.slot is None:
                del _registry[key]
        return
    for p in params:
        if p.dim() == 4:
            o = p.untyped_storage().data_ptr()
            _register(p).reset(_owners.get(o) or _owners.setdefault(o, _Owner(o)))


def weights_changed(flat=None):
    """Invalidate the cached derived tensors (packed operands, squared-weight sums) of the weights living in the flat
    buffer `flat` (a tensor) -- or of all registered weights.  Called by the fused optimizer / EMA kernels, which
    update parameters through raw pointers (no version counter moves)."""
    if flat is not None:
        own = _owners.get(flat.untyped_storage().data_ptr())
        if own is not None:
            own.gen += 1
        return
    for own in _owners.values():
        own.gen += 1
    if any(own.events for own in _owners.values()) and not torch.cuda.is_current_stream_capturing():
        drain_pack_streams()


def cached(w, tag, compute):
    """compute(w) cached per registered weight and `tag` until that weight's buffer changes; uncached otherwise."""
    rec = record(w)
    if rec is None or rec.owner is None:
        return compute(w)
    own = rec.owner
    st = (own.gen, w._version)
    if rec.stamp == st and tag in rec.vals:
        if tag == 'wsq':
            _await_pack(own, w.device, rec.key)
        return rec.vals[tag]
    # the batched packing launch of this weight's flat buffer also leaves sum_taps W^2 of every weight (hg_pack_item.wsq)
    if tag == 'wsq' and w.is_cuda and _pack_owner(own, w.device) and rec.stamp == st and tag in rec.vals:
        return rec.vals[tag]
    val = compute(w)
    rec.restamp(st)
    rec.vals[tag] = val
    return val


class Operand:
    """A packed convolution weight as the launch wrappers take it."""
    __slots__ = ('direct', 'winograd', 'mode', 'src', 'rec', 'stale', 'wino_pending')

    def __init__(self, direct, mode, src, rec=None, wino=None, wino_pending=False):
        self.direct, self.mode = direct, mode    # Wt[k*k][Kp][Np] of hg_conv2d_fwd / hg_conv2d_dgrad
        self.winograd = wino                # the Winograd operand of hg_wino_conv2d, or None
        self.src, self.rec = src, rec       # what it is packed from: a weakref (registered weight, its record) or the tensor
        self.stale = False                  # `direct` was left out of the batched pack: direct_operand packs it
        self.wino_pending = wino_pending    # per-call operand of a 3x3 weight: `winograd` is packed by the first launch that takes it


def pack_weights(w, mode):
    """(Co,Ci,k,k) -> the packed Operand of hg_conv2d_fwd / hg_conv2d_dgrad (and of their Winograd forms)."""
    rec = record(w)
    if rec is None or rec.owner is None:
        return Operand(_pack_weights(w, mode), mode, w, wino_pending=w.shape[2] == 3)
    own = rec.owner
    st = (own.gen, w._version)
    if rec.stamp == st and rec.ops[mode] is not None:
        _await_pack(own, w.device, rec.key)
        return rec.ops[mode]
    # A registered (training) weight needs both operands once per optimizer step, and so do all its siblings in the
    # same flat buffer: ONE launch packs every convolution weight of that buffer (hg_conv_pack_weights_multi) the
    # first time one of them is asked for after the buffer changed.
    if _pack_owner(own, w.device) and rec.stamp == st and rec.ops[mode] is not None:
        return rec.ops[mode]
    rec.restamp(st)
    rec.ops = [Operand(t, m, rec.ref, rec, wino_pending=w.shape[2] == 3) for m, t in enumerate(_pack_both(w))]
    return rec.ops[mode]


def wino_operand(op, B, K, N, H, W):
    """The Winograd buffer of `op` for this launch, or None (direct kernel)."""
    if not wino_supported(B, K, N, H, W):
        return None
    if op.rec is not None:
        op.rec.wants_wino = True
    if op.wino_pending:
        op.wino_pending = False
        u = _wino_pack(op.src if op.rec is None else op.src(), op.mode)
        op.winograd = None if u is False else u
    return op.winograd


def direct_operand(op):
    """The direct buffer of `op` for a launch: packed now if the batched pack left it out (plan_weights)."""
    rec = op.rec
    if rec is not None:
        rec.wants_direct = True      # into the batched launch from the next plan on
    if op.stale:
        p = op.src()
        if p is None:       # (an operand outliving its weight: nothing to pack from -- never hand a stale buffer to a launch)
            raise RuntimeError('direct convolution operand requested for a weight that no longer exists')
        Co, Ci, k, _ = p.shape
        with on_device(p.device):
            check(lib.hg_conv_pack_weights(p.data_ptr(), op.direct.data_ptr(), Co, Ci, k, op.mode, stream_of(p)), 'hg_conv_pack_weights')
        op.stale = False
        if rec.owner is not None and not torch.cuda.is_current_stream_capturing():
            # another stream that takes this operand afterwards sees stale == False: it has to wait for THIS pack
            # (registered like the batched pack: consumers wait once per stream, _await_pack)
            cur = torch.cuda.current_stream(p.device)
            rec.owner.events.append([cur.record_event(), {cur.cuda_stream}, {rec.key}])
    return op.direct


# ---- the batched pack: plan, build, launch -------------------------------------------------------------------------
class _PackItem(ctypes.Structure):       # include/hg_conv.h: hg_pack_item
    _fields_ = [('w', ctypes.c_void_p), ('wt_fwd', ctypes.c_void_p), ('wt_dgrad', ctypes.c_void_p),
                ('Co', ctypes.c_int32), ('Ci', ctypes.c_int32), ('ksize', ctypes.c_int32), ('block_begin', ctypes.c_int32),
                ('wsq', ctypes.c_void_p)]


class _WinoItem(ctypes.Structure):       # include/hg_wino.h: hg_wino_pack_item
    _fields_ = [('w', ctypes.c_void_p), ('u_fwd', ctypes.c_void_p), ('u_dgrad', ctypes.c_void_p), ('wsq', ctypes.c_void_p),
                ('Co', ctypes.c_int32), ('Ci', ctypes.c_int32), ('block_begin', ctypes.c_int32), ('reserved', ctypes.c_int32)]


# What the batched pack does for one weight.  block: first block of its item in hg_conv_pack_weights_multi, None = no item
# (its direct operands stay stale until a launch asks for them); nf, nd: elements of its Winograd forward / data-gradient operands
# (0: none); wblock: first block of its item in hg_wino_pack_weights_multi, None = no item; wsq: the item that writes
# sum_taps W^2 (the demodulation coefficient's weight factor), 'direct' or 'wino'.
Packed = collections.namedtuple('Packed', 'key block nf nd wblock wsq')


def plan_weights(recs, wino):
    """The batched pack of the records `recs` (one flat buffer's live weights): (a Packed per weight -- the plan's signature --,
    blocks of the direct launch, blocks of the Winograd launch).  Host logic only.  A 3x3 weight gets Winograd operands unless its
    launches only ever took the direct one (the discriminator's stride-2 convolutions, layers hg_wino_supported refuses: 16/9 of the
    weight per mode, re-packed every step for nobody); with both, and no launch that took the direct one, it needs no direct pack."""
    out, blocks, wblocks = [], 0, 0
    for rec in recs:
        if rec.geom is None:
            Co, Ci, k, _ = rec.key[1]
            nf, nd = (lib.hg_wino_packed_elems(Co, Ci, m) if k == 3 else 0 for m in (PACK_FWD, PACK_DGRAD))
            rec.geom = (nf, nd, lib.hg_conv_pack_blocks(Co, Ci),
                        lib.hg_wino_pack_blocks(Co, Ci, int(bool(nf)), int(bool(nd))) if nf or nd else 0)
        nf, nd, nb, nwb = rec.geom
        if not wino or (rec.wants_direct and not rec.wants_wino):
            nf = nd = nwb = 0
        lazy = bool(nf and nd and not rec.wants_direct)
        out.append(Packed(rec.key, None if lazy else blocks, nf, nd, wblocks if nf or nd else None, 'wino' if lazy else 'direct'))
        blocks += 0 if lazy else nb
        wblocks += nwb
    return tuple(out), blocks, wblocks


# The buffers and device tables of one flat buffer's batched pack.  ops: key -> ([forward, data-gradient Operand], wsq); lazy:
# the Operands the direct launch leaves out; direct, wino: (device table, items, blocks) of a launch, or None.
_Plan = collections.namedtuple('_Plan', 'sig ops lazy direct wino')


def _build_plan(sig, blocks, wblocks, live, device):
    """Allocate the operand buffers of plan `sig` and upload its two item tables."""
    ops, lazy, items, witems = {}, [], [], []
    new = lambda *n: torch.empty(n, dtype=torch.float32, device=device)
    for it, (rec, p) in zip(sig, live):
        Co, Ci, k, _ = p.shape
        wf, wd = (new(lib.hg_conv_packed_elems(Co, Ci, k, m)) for m in (PACK_FWD, PACK_DGRAD))
        uf, ud, wq = new(it.nf) if it.nf else None, new(it.nd) if it.nd else None, new(Co, Ci)
        pair = [Operand(wf, PACK_FWD, rec.ref, rec, uf), Operand(wd, PACK_DGRAD, rec.ref, rec, ud)]
        ops[it.key] = (pair, wq)
        if it.block is None:
            lazy += pair
        else:
            items.append(_PackItem(p.data_ptr(), wf.data_ptr(), wd.data_ptr(), Co, Ci, k, it.block,
                                   wq.data_ptr() if it.wsq == 'direct' else None))
        if it.wblock is not None:
            witems.append(_WinoItem(p.data_ptr(), ptr(uf), ptr(ud), wq.data_ptr() if it.wsq == 'wino' else None, Co, Ci, it.wblock, 0))
    up = lambda arr: torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone().to(device)
    return _Plan(sig, ops, lazy, (up((_PackItem * len(items))(*items)), len(items), blocks) if items else None,
                 (up((_WinoItem * len(witems))(*witems)), len(witems), wblocks) if witems else None)


def _pack_owner(own, device, launch=True, record_on=None):
    """Pack every live registered weight of flat buffer `own` into persistent operand buffers (direct operands + squared
    sums: hg_conv_pack_weights_multi; Winograd operands of the 3x3 weights: hg_wino_pack_weights_multi) and stamp their
    records.  One pair of launches per buffer (packing a leading share of the weights first was measured without gain: 789.9
    against 793.7 images/s, profiles/r05_ab_pack_split.json).  `record_on`: the stream the launches run on -- an event is
    recorded there for the consumers (_await_pack).  The plan is rebuilt when plan_weights decides differently."""
    live = []
    for rec in list(_registry.values()):
        p = rec.ref()
        if rec.owner is own and p is not None and p.data_ptr() == rec.key[0] and p.is_cuda and p.device == device \
                and p.dtype == torch.float32 and p.is_contiguous() and p.shape[2] == p.shape[3] and p.shape[2] in (1, 3):
            live.append((rec, p))
    if not live:
        return False
    sig, blocks, wblocks = plan_weights([rec for rec, _ in live], WINO)
    plan = own.plan
    with on_device(device):
        if plan is None or plan.sig != sig:
            if torch.cuda.is_current_stream_capturing():
                return False          # (the table upload is not capturable: per-weight launches for this capture)
            plan = own.plan = _build_plan(sig, blocks, wblocks, live, device)
        if not launch:
            return True
        _await_pack(own, device)           # an asynchronous pack of the same buffers still in flight goes first
        own.events = []
        for op in plan.lazy:               # (weights changed: a direct operand packed on demand last step is stale again)
            op.stale = True
        for name, tab in (('hg_conv_pack_weights_multi', plan.direct), ('hg_wino_pack_weights_multi', plan.wino)):
            if tab is not None:
                table, n, nblocks = tab
                check(getattr(lib, name)(table.data_ptr(), n, nblocks, raw_stream(device)), name)
        if record_on is not None:
            own.events = [[record_on.record_event(), {record_on.cuda_stream}, plan.ops]]
    for rec, p in live:
        rec.stamp = (own.gen, p._version)
        rec.ops, wq = plan.ops[rec.key]
        rec.vals = {'wsq': wq}
        for op in rec.ops:      # (a plan outlives a freed model whose successor's weights land at the same addresses)
            op.rec, op.src = rec, rec.ref
    return True


def build_pack_plans(device):
    """Build the batched-pack plans of every registered flat buffer now (allocations + one small host-to-device copy each),
    e.g. before a hipGraph capture, inside which a plan cannot be built."""
    for own in list(_owners.values()):
        _pack_owner(own, device, launch=False)


def prepack_async(flat):
    """Pack the convolution weights of flat buffer `flat` NOW, on a stream of its own, instead of at their first use: after the
    generator's optimizer step that first use is the first convolution of the next step's generator forward, behind the
    mapping network's serial ~15 us launches -- the 0.2 ms packing launch runs under those.  Consumers wait for the pack's
    event (_await_pack, once per stream); the launch itself is ordered behind everything enqueued on the current stream
    (the readers of the operand buffers it overwrites)."""
    own = _owners.get(flat.untyped_storage().data_ptr())
    if own is None or not flat.is_cuda or torch.cuda.is_current_stream_capturing():
        return False
    st = _device_stream('pack', flat.device)
    st.wait_event(torch.cuda.current_stream(flat.device).record_event())
    with torch.cuda.stream(st):
        return _pack_owner(own, flat.device, record_on=st)


def drain_pack_streams():
    """The current stream of every device waits for its asynchronous pack stream, and the per-owner pack events are dropped:
    called before a train-step graph is captured / replayed (a capturing stream must not wait on an event recorded outside the
    capture) and when every cached operand is invalidated from the host (weights_changed(None): the next pack of the same
    buffers then runs behind the one in flight)."""
    for (kind, idx), st in _streams.items():
        if kind == 'pack':
            torch.cuda.current_stream(torch.device('cuda', idx)).wait_stream(st)
    for own in _owners.values():
        own.events = []


def _await_pack(own, device, key=None):
    """The current stream waits for the asynchronous packs of flat buffer `own` -- for those that cover weight `key`
    (None: all of them) -- once per stream and event."""
    if not own.events or torch.cuda.is_current_stream_capturing():    # (drain_pack_streams() ran before the capture began)
        return
    cur = torch.cuda.current_stream(device)
    for ev, seen, keys in own.events:
        if (key is None or key in keys) and cur.cuda_stream not in seen:
            cur.wait_event(ev)
            seen.add(cur.cuda_stream)


# ---- weight gradients straight into the optimizer's flat gradient buffer, on a side stream ----------------------
# In a plain backward pass (no graph being built) the weight gradient of a registered convolution weight is not
# handed to autograd at all: k_wgrad writes it into the weight's slice of the flat gradient buffer (optim.FlatParams)
# on a SIDE stream.  (i) no per-parameter copy into the flat buffer afterwards; (ii) the MFMA-bound weight-gradient
# kernel runs beside the HBM-bound elementwise kernels that follow the convolution in the backward pass (LeakyReLU /
# modulation / demodulation gradients, residual adds): measured 50 % of their time hidden (tools/overlap_probe.py).
# All direct writes go through the one side stream, in order, so a second contribution to the same weight in the same
# step (gradient accumulation, the gradient penalty's second-order term, the path-length pass) is simply added there;
# FlatParams.gather() makes the main stream wait for the side stream before anything reads the buffer.
def register_grad_slots(flat):
    """Called by FlatParams: convolution weights (4-d parameters) of `flat` may receive their gradient directly.
    Only a weak reference to the owner is kept."""
    ref = weakref.ref(flat)
    for p, s in zip(flat.params, flat.slots):
        if p.dim() == 4:
            _register(p).slot = (ref, s.index)


def grad_slot(w):
    """(slot view, owner FlatParams, slot already written this step, slot index for the owner's mark_written()) of a registered
    convolution weight whose gradient may be written directly right now (between zero_grad() and gather(), plain backward), or None."""
    rec = None if torch.is_grad_enabled() else record(w)
    if rec is None or rec.slot is None:
        return None
    ref, index = rec.slot
    flat = ref()
    return None if flat is None else flat.slot(index)


side_stream = functools.partial(_device_stream, 'wgrad')


def on_wgrad_stream(device, run, reads):
    """run() on the weight-gradient stream, behind everything enqueued on the current stream; `reads`: the tensors it reads
    (the caching allocator must not recycle them under the kernel).  Overwrite-vs-accumulate of a flat gradient slot is decided
    from the owner's host-side set of written slot indices (`FlatParams.written`) at ENQUEUE time: every direct write goes through
    here, onto ONE stream in order.
    Inside a hipGraph capture every fork to the side stream becomes a cross-branch dependency edge (~100 per step): measured
    slower than the eager side stream; the direct write (no per-parameter copy) stays, on the capturing stream."""
    if torch.cuda.is_current_stream_capturing():
        return run()
    side = side_stream(device)
    side.wait_event(torch.cuda.current_stream(device).record_event())
    with torch.cuda.stream(side):
        run()
    for t in reads:
        t.record_stream(side)
