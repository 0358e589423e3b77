"""Flat parameter storage, fused DiffGrad and fused EMA (hg_diffgrad_step / hg_ema_update).

MI355X-first layout: every optimizer owns ONE contiguous fp32 parameter buffer and ONE contiguous
gradient buffer (parameters / .grad are views into them).  One kernel launch updates all parameters,
one (or a few large) collectives reduce all gradients, EMA is one launch -- instead of ~12 aten
launches per parameter tensor (reference: torch_optimizer.DiffGrad over ~150 tensors, and the
per-tensor EMA loop of histoGAN/histoGAN.py:698-707).
"""
import collections

import torch

from ._lib import check, lib, on_device, stream_of
from .wpack import register_grad_slots, side_stream, weights_changed


def conv_first(params):
    """`params` with the convolution weights (4-d tensors) first, order otherwise kept: the flat buffer then starts with one
    contiguous region that holds every convolution weight (FlatParams.n_conv elements) -- the region whose gradients are final
    when the last convolution's backward has been enqueued, long before the mapping networks' (ddp.GradAllReduce.start_early)."""
    params = list(params)
    return [p for p in params if p.dim() == 4] + [p for p in params if p.dim() != 4]


# One row of FlatParams.slots: parameter `index` lives at elements [offset, offset + numel) of the flat buffers; `view`: the
# persistent view of that range of the gradient buffer, in the parameter's shape (None without a gradient buffer).
Slot = collections.namedtuple('Slot', 'index offset numel view')

# The phases of a step's gradients (FlatParams.phase).  OPEN: between zero_grad() and gather() / close(), convolution weights
# may get their gradient written straight into their slot; CLOSED: no more direct writes, gather() still to come; GATHERED:
# the flat gradient buffer and every p.grad hold the step's gradients.
CLOSED, OPEN, GATHERED = 'closed', 'open', 'gathered'


class FlatParams:
    """Re-home `params` (already on their final device) into one flat buffer; optionally with grads.  `slots` is THE layout:
    the parameter / gradient views, `n_conv` and the direct-write registration (wpack.register_grad_slots) all come from it."""

    def __init__(self, params, with_grad=True):
        self.params = list({id(p): p for p in params}.values())       # (a parameter given twice is kept once, order kept)
        if not self.params:
            raise ValueError('no parameters')
        dev = self.params[0].device
        self.numel = sum(p.numel() for p in self.params)
        self.data = torch.empty(self.numel, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(self.numel, dtype=torch.float32, device=dev) if with_grad else None
        # persistent views of every parameter's slice of the gradient buffer (gather() runs twice per step over ~150
        # parameters: slicing + viewing them anew cost the host ~1.5 ms per call)
        self.slots = []
        off = 0
        for i, p in enumerate(self.params):
            n = p.numel()
            self.slots.append(Slot(i, off, n, self.grad[off:off + n].view(p.shape) if with_grad else None))
            view = self.data[off:off + n].view(p.shape)
            view.copy_(p.data)
            p.data = view
            if with_grad:
                p.grad = self.slots[i].view
            off += n
        lead = next((s for p, s in zip(self.params, self.slots) if p.dim() != 4), None)
        self.n_conv = self.numel if lead is None else lead.offset       # elements of the leading run of 4-d parameters
        # per-step state.  Convolution weights may get their gradient written straight into their slot (conv._direct_wgrad)
        self.generation = 0        # the step: incremented by zero_grad()
        self.phase = GATHERED      # (before the first zero_grad() the buffers are consistent: gather() has nothing to do)
        self.written = set()       # indices of the slots written directly in this generation
        if with_grad:
            register_grad_slots(self)

    def slot(self, index):
        """(slot view, self, slot already written this step, index) while direct writes are accepted, else None (wpack.grad_slot)."""
        if self.phase != OPEN:
            return None
        return self.slots[index].view, self, index in self.written, index

    def mark_written(self, index):
        """Slot `index` holds a gradient of this step, written directly: the next direct write adds to it, gather() keeps it."""
        self.written.add(index)

    def conv_region_final(self):
        """True when every parameter of the leading convolution-weight region (n_conv elements) has its gradient of this step
        in its flat slot, written directly (conv._direct_wgrad, the demodulation term, gfused's to-RGB write) and by nothing
        else -- the condition under which that region may be reduced / updated before gather()."""
        if self.n_conv <= 0 or self.phase != OPEN or self.grad is None:
            return False
        return all(s.index in self.written and p.grad is None for p, s in zip(self.params, self.slots) if s.offset < self.n_conv)

    def zero_grad(self):
        """Drop the parameter gradients.  With `.grad = None` autograd's AccumulateGrad hands over the incoming gradient
        tensor instead of launching one `grad += new` kernel per parameter into a zeroed buffer; `gather()` then
        copies all of them into the flat gradient buffer with a few multi-tensor launches."""
        for p in self.params:
            p.grad = None
        self.generation += 1
        self.written = set()
        self.phase = OPEN

    def close(self):
        """Stop accepting direct writes (wpack.grad_slot answers None from here on); gather() is still to come."""
        if self.phase == OPEN:
            self.phase = CLOSED

    def gather(self):
        """Make `self.grad` (and every `p.grad`, re-pointed to its slice) hold the gradients of the last backward
        passes; parameters that received none get zeros.  Idempotent."""
        if self.phase == GATHERED:
            return
        self.close()
        # weight gradients written on the side stream: order them before any reader (captured: written on this branch)
        if self.written and self.grad.is_cuda and not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream(self.grad.device).wait_stream(side_stream(self.grad.device))
        dst, src, missing, both = [], [], [], []
        for p, (i, _, _, v) in zip(self.params, self.slots):
            pg = p.grad
            if i in self.written:
                if pg is not None and pg is not v and pg.data_ptr() != v.data_ptr():
                    both.append((v, pg))           # autograd ALSO delivered a part (a pass that recorded a graph)
            elif pg is None:
                missing.append(v)
            elif pg is not v and pg.data_ptr() != v.data_ptr():
                dst.append(v)
                src.append(pg)
            if pg is not v:
                p.grad = v
        if dst:
            torch._foreach_copy_(dst, src)
        if missing:
            torch._foreach_zero_(missing)
        if both:
            torch._foreach_add_([v for v, _ in both], [g for _, g in both])
        self.phase = GATHERED


class DiffGrad:
    """DiffGrad (Dubey et al.; torch_optimizer.DiffGrad as used at histoGAN/histoGAN.py:670-671) over a
    FlatParams: p -= lr*sqrt(1-b2^t)/(1-b1^t) * (m * dfc) / (sqrt(v)+eps), dfc = sigmoid(|g_prev - g|)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.flat = params if isinstance(params, FlatParams) else FlatParams(params)
        self.lr, self.betas, self.eps = lr, betas, eps
        self.step_count = 0
        self.graph_mode = False
        self._step_size_dev = None
        z = lambda: torch.zeros_like(self.flat.data)
        self.exp_avg, self.exp_avg_sq, self.previous_grad = z(), z(), z()
        self.param_groups = [{'params': self.flat.params, 'lr': lr, 'betas': betas, 'eps': eps}]

    def zero_grad(self, set_to_none=False):
        self.flat.zero_grad()

    def prepare_replay(self):
        """Graph mode (the train step captured as a hipGraph): advance the step counter on the host and refresh the
        bias-corrected step size the captured launch reads from device memory.  Call once per replay, before it."""
        self.step_count += 1
        if self._step_size_dev is None:
            self._step_size_dev = torch.zeros((), dtype=torch.float32, device=self.flat.data.device)
        lr = self.param_groups[0]['lr']
        self._step_size_dev.fill_(lib.hg_diffgrad_step_size(float(lr), float(self.betas[0]), float(self.betas[1]),
                                                            self.step_count))

    def step_buckets(self, reducer):
        """The update bucket by bucket behind a bucketed gradient all-reduce (ddp.GradAllReduce, already started): bucket
        i's parameters are updated as soon as ITS collective is done, while the later buckets are still on the wire.
        Elementwise over the flat buffer: the same update as one launch."""
        f = self.flat
        f.gather()
        if not f.data.is_cuda:
            raise RuntimeError('DiffGrad: parameters are not on a GPU; no CPU implementation')
        if self.graph_mode:
            raise RuntimeError('DiffGrad.step_buckets: not available inside a captured graph')
        self.step_count += 1
        with on_device(f.data.device):
            for i, (lo, hi) in enumerate(reducer.ranges):
                reducer.wait(i)
                self._launch(lo, hi, self.step_count)
        reducer.finish()
        weights_changed(f.data)

    def _buffers(self, lo=0):
        """Addresses of element `lo` of the five flat buffers, in the order the step kernels take them."""
        f = self.flat
        return [t.data_ptr() + 4 * lo for t in (f.data, f.grad, self.exp_avg, self.exp_avg_sq, self.previous_grad)]

    def _launch(self, lo, hi, step_count):
        """hg_diffgrad_step over elements [lo, hi) of the flat buffers, as step number `step_count`."""
        f = self.flat
        lr = self.param_groups[0]['lr']
        with on_device(f.data.device):
            check(lib.hg_diffgrad_step(*self._buffers(lo), hi - lo, float(lr), float(self.betas[0]), float(self.betas[1]),
                                       float(self.eps), step_count, stream_of(f.data)), 'hg_diffgrad_step')

    def step(self):
        f = self.flat
        f.gather()
        if not f.data.is_cuda:
            raise RuntimeError('DiffGrad: parameters are not on a GPU; no CPU implementation')
        if self.graph_mode:           # being captured: step size from device memory, counter advanced by prepare_replay()
            with on_device(f.data.device):
                check(lib.hg_diffgrad_step_dev(*self._buffers(), f.numel, self._step_size_dev.data_ptr(), float(self.betas[0]),
                                               float(self.betas[1]), float(self.eps), stream_of(f.data)),
                      'hg_diffgrad_step_dev')
        else:
            self.step_count += 1
            self._launch(0, f.numel, self.step_count)
        weights_changed(f.data)


def ema_update(ma_flat, cur_flat, beta):
    """ma = beta*ma + (1-beta)*cur over two FlatParams with identical layout (HistoGAN.EMA)."""
    if ma_flat.numel != cur_flat.numel:
        raise ValueError('EMA buffers differ in size')
    with on_device(ma_flat.data.device):
        check(lib.hg_ema_update(ma_flat.data.data_ptr(), cur_flat.data.data_ptr(), ma_flat.numel, float(beta),
                                stream_of(ma_flat.data)), 'hg_ema_update')
    weights_changed(ma_flat.data)
