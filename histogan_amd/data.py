"""Image-folder source and image-grid writer (PIL only; torchvision is absent in this image).

The reference's Dataset (histoGAN/histoGAN.py:253-307, ReHistoGAN/rehistoGAN.py:335-446) decodes with PIL/torchvision in
DataLoader workers and computes TWO CPU target histograms of full-resolution images per item (~1 s each on the
reference's fp64 CPU path): at the 470 images/s of the GPU step that pipeline would starve the GPU by three orders of
magnitude.  This source keeps the item contract -- {'images': (B,3,S,S) in [0,1],
'histograms': interpolation of the histograms of two other random images, or the image's own} -- and restructures it:

* decoding / resizing runs in a thread pool (PIL releases the GIL) and batches are prefetched `prefetch` deep;
* target histograms are computed on the GPU (one launch per full-resolution image, sizes differ) and CACHED per
  image on the device: the histogram of image i never changes, so after the first pass over the folder a batch's
  targets are two gathers and one interpolation -- the reference's "precompute histograms.npy" flow
  (create_hist_data.py:33-55) done lazily;
* nothing touches the CPU histogram path.

ResidentFolderData (opt-in) goes one step further: every file is decoded once and its resized uint8 image stays on the
device, where the kernels of include/hg_data.h crop, resize, flip and convert each batch -- the same batches, bit for bit
(pil_bilinear_tables restates Pillow's integer resize).
"""
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache
from pathlib import Path

import numpy as np
import torch

EXTS = ['jpg', 'png']


def _random_resized_crop_box(w, h, rs, scale=(0.5, 1.0), ratio=(0.98, 1.02)):
    """torchvision.transforms.RandomResizedCrop.get_params restated (histoGAN/histoGAN.py:277-279 uses scale (0.5, 1),
    ratio (0.98, 1.02)): up to 10 draws of (area fraction, log-uniform aspect), then the ratio-clamped centre crop."""
    area = w * h
    lr = np.log(ratio)
    for _ in range(10):
        target = area * rs.uniform(scale[0], scale[1])
        ar = np.exp(rs.uniform(lr[0], lr[1]))
        cw, ch = int(round(np.sqrt(target * ar))), int(round(np.sqrt(target / ar)))
        if 0 < cw <= w and 0 < ch <= h:
            return int(rs.randint(0, w - cw + 1)), int(rs.randint(0, h - ch + 1)), cw, ch
    in_ratio = w / h
    if in_ratio < ratio[0]:
        cw, ch = w, int(round(w / ratio[0]))
    elif in_ratio > ratio[1]:
        cw, ch = int(round(h * ratio[1])), h
    else:
        cw, ch = w, h
    return (w - cw) // 2, (h - ch) // 2, cw, ch


def _load_rgb(path, size=None, flip=False, rgba=False, crop_seed=None):
    """crop_seed: None = Resize + CenterCrop; an int = Resize + RandomResizedCrop(size, scale (0.5,1), ratio (0.98,1.02))
    drawn from that seed (the `dataset_aug_prob` branch of the reference's transform, histoGAN/histoGAN.py:273-283)."""
    from PIL import Image
    img = Image.open(path).convert('RGBA' if rgba else 'RGB')    # convert_rgb_to_transparent / _transparent_to_rgb
    if size is not None:
        w, h = img.size
        # transforms.Resize(size) (after resize_to_minimum_size, which is the same call for small images, :246-249): short
        # side -> size, long side int(size * long / short) -- torchvision TRUNCATES -- and no-op when the short side matches
        short, long = (w, h) if w <= h else (h, w)
        if short != size:
            new_long = int(size * long / short)
            img = img.resize((size, new_long) if w <= h else (new_long, size), Image.BILINEAR)
        w, h = img.size
        if crop_seed is None:
            # transforms.CenterCrop(size): torchvision's offsets are int(round((dim - size) / 2.0)) (round half to even)
            l, t = int(round((w - size) / 2.0)), int(round((h - size) / 2.0))
            img = img.crop((l, t, l + size, t + size))
        else:
            l, t, cw, ch = _random_resized_crop_box(w, h, np.random.RandomState(crop_seed))
            img = img.resize((size, size), Image.BILINEAR, box=(l, t, l + cw, t + ch))
    arr = np.asarray(img, dtype=np.float32) / 255.0            # ToTensor
    if flip:
        arr = arr[:, ::-1]                                     # transforms.RandomHorizontalFlip
    return torch.from_numpy(np.ascontiguousarray(arr)).permute(2, 0, 1).contiguous()


class FolderData:
    def __init__(self, folder, hist_block, batch_size, image_size, device, transparent=False, seed=0, test=False,
                 hist_sampling=True, workers=8, prefetch=3, cache_hists=True, max_cached=200000, hflip=False,
                 aug_prob=0.0, max_cache_bytes=2 << 30, hist_alpha_weight=False):
        self.rgba = bool(transparent)                            # 4-channel items; the histogram uses channels 0..2
        # opt-in: the target histograms weigh every pixel by its alpha (channel 3), so the colour stored under transparent
        # pixels does not count; default: alpha is ignored, as in the reference
        if hist_alpha_weight and not transparent:
            raise ValueError('hist_alpha_weight=True needs transparent=True (there is no alpha channel to weigh by)')
        self.alpha_weight = bool(hist_alpha_weight)
        self.paths = sorted(p for ext in EXTS for p in Path(f'{folder}').glob(f'**/*.{ext}'))
        if not self.paths:
            raise FileNotFoundError(f'no {EXTS} images under {folder}')
        self.hist_block, self.B, self.S, self.device, self.test = hist_block, batch_size, image_size, device, test
        self.rs = np.random.RandomState(seed)
        # True: target = interpolation of the histograms of two OTHER random images; False: the image's own
        # histogram (ReHistoGAN/rehistoGAN.py:375-446, `hist_sampling`)
        self.hist_sampling = hist_sampling
        self.hflip = hflip                                      # the reference's training transform flips with p = 0.5
        self.aug_prob = float(aug_prob)                         # `dataset_aug_prob`: P(RandomResizedCrop instead of CenterCrop)
        self.cache = {} if cache_hists else None
        self.max_cached = max_cached
        self.max_cache_bytes, self.cache_bytes = int(max_cache_bytes), 0   # device memory the cached histograms may take
        self.pool = ThreadPoolExecutor(max_workers=max(1, workers))
        self.queue = deque()
        self.prefetch = max(1, prefetch)
        self.hits = self.misses = 0

    # ---- planning (host RNG, main thread: deterministic for a seed) and decoding (worker threads)
    def _plan(self):
        n = len(self.paths)
        plan = {'img': self.rs.randint(0, n, self.B)}
        own = self.test or not self.hist_sampling              # target = the image's own histogram
        if not own:
            plan['h1'], plan['h2'] = self.rs.randint(0, n, self.B), self.rs.randint(0, n, self.B)
            plan['ratio'] = self.rs.rand(self.B).astype(np.float32)       # hist_interpolation (:180-182), per item
        flips = self.rs.rand(self.B) < 0.5 if (self.hflip and not self.test) else np.zeros(self.B, bool)
        need = set(int(i) for key in (('img',) if own else ('h1', 'h2')) for i in plan[key])
        if self.cache is not None:
            need = {i for i in need if i not in self.cache}
        plan['full'] = self._full_jobs(sorted(need))
        crops = [int(self.rs.randint(0, 2 ** 31 - 1)) if (self.aug_prob > 0.0 and not self.test and self.rs.rand() < self.aug_prob)
                 else None for _ in range(self.B)]
        plan['small'] = None if self.test else self._small_jobs(plan['img'], flips, crops)
        return plan

    # what a plan starts in the pool (ResidentFolderData starts one uint8 decode per file instead)
    def _full_jobs(self, need):
        return {i: self.pool.submit(_load_rgb, self.paths[i], None, False, self.rgba) for i in need}   # full resolution

    def _small_jobs(self, img, flips, crops):
        return [self.pool.submit(_load_rgb, self.paths[int(i)], self.S, bool(f), self.rgba, c) for i, f, c in zip(img, flips, crops)]

    def _hist(self, idx, plan):
        """(len(idx), 3, h, h) target histograms on the device: cached, or one GPU launch per missing image."""
        out = []
        for i in (int(v) for v in idx):
            h = self.cache.get(i) if self.cache is not None else None
            if h is None:
                h = self._miss(i, plan)
            else:
                self.hits += 1
            out.append(h)
        return torch.stack(out)

    def _miss(self, i, plan):
        fut = plan['full'].get(i)
        x = (fut.result() if fut is not None else _load_rgb(self.paths[i], None, False, self.rgba)).unsqueeze(0).to(self.device)
        return self._new_hist(i, x)

    def _new_hist(self, i, x):
        """The target histogram of image i from its full-resolution batch of one; counted, and cached while there is room."""
        with torch.no_grad():
            h = (self.hist_block(x, weight=x[:, 3]) if self.alpha_weight else self.hist_block(x))[0]
        self.misses += 1
        nbytes = h.numel() * h.element_size()
        if self.cache is not None and len(self.cache) < self.max_cached and \
                self.cache_bytes + nbytes <= self.max_cache_bytes:
            self.cache[i] = h
            self.cache_bytes += nbytes
        return h

    def __iter__(self):
        return self

    def __next__(self):
        while len(self.queue) < self.prefetch:
            self.queue.append(self._plan())
        plan = self.queue.popleft()
        batch = {}
        if plan['small'] is not None:
            host = torch.stack([f.result() for f in plan['small']])
            batch['images'] = host.pin_memory().to(self.device, non_blocking=True) if self.device.type == 'cuda' \
                else host.to(self.device)
        ratio = torch.from_numpy(plan['ratio']).to(self.device) if 'h1' in plan else None
        batch['histograms'] = self._targets(plan, ratio)
        return batch

    def _targets(self, plan, ratio):
        """The batch's target histograms; ratio: plan['ratio'] on the device (interpolated targets), else None."""
        if ratio is None:
            return self._hist(plan['img'], plan)
        ratio = ratio.view(-1, 1, 1, 1)
        return self._hist(plan['h1'], plan) * ratio + self._hist(plan['h2'], plan) * (1 - ratio)


# ---- Pillow's uint8 bilinear resize, restated for the device (include/hg_data.h) ---------------------------------------------
PRECISION_BITS = 32 - 8 - 2          # Pillow's 8-bit resample: coefficients are fixed point with 22 fractional bits


@lru_cache(maxsize=512)
def pil_bilinear_tables(in_size, in0, in1, out_size):
    """One axis of `Image.resize(..., Image.BILINEAR, box=...)` on an 8-bit image as integer tables: (bounds int32
    (out_size, 2) = (first input, taps) per output position, coeffs int32 (out_size, ksize) = round(weight * 2^22), zero past
    a row's taps).  in_size: the axis' length; [in0, in1): the box along it.  The output byte is
    clip((2^21 + sum_t coeffs[o, t] * pix[first + t]) >> 22, 0, 255).  fp64, as Pillow computes them, after the box has gone
    through float32 as it does there; the arrays are cached and read-only."""
    in_size, out_size, in0, in1 = int(in_size), int(out_size), float(in0), float(in1)
    if in_size < 1 or out_size < 1 or not in0 < in1:
        raise ValueError(f'pil_bilinear_tables: an axis of {in_size} with box [{in0}, {in1}) to {out_size} outputs')
    f0, f1 = np.float32(in0), np.float32(in1)                   # Pillow's C entry point takes the box as four floats ...
    scale, in0 = float(f1 - f0) / out_size, float(f0)           # ... and subtracts them as floats; fp64 from here on
    filterscale = max(scale, 1.0)
    support = filterscale                                       # bilinear: support 1 x filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    center = in0 + (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)            # C's (int): truncation
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    a = np.abs((x + xmin[:, None] - center[:, None] + 0.5) / filterscale)
    w = np.where((a < 1.0) & (x < xmax[:, None]), 1.0 - a, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                           # left to right, as the C loop adds them
    w = np.divide(w, ww, out=w, where=ww != 0.0)
    coeffs = (0.5 + w * float(1 << PRECISION_BITS)).astype(np.int64).astype(np.int32)
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return bounds, coeffs


def stage1_size(w, h, size):
    """transforms.Resize(size) as `_load_rgb` applies it: the short side -> size, the long side int(size * long / short)."""
    short, long = (w, h) if w <= h else (h, w)
    if short == size:
        return w, h
    new_long = int(size * long / short)
    return (size, new_long) if w <= h else (new_long, size)


ITEM_DTYPE = np.dtype([('src', '<u8'), ('dst', '<u8'), ('src_stride', '<i8'), ('dst_stride', '<i8'), ('n_out', '<i4'),
                       ('n_keep', '<i4'), ('tab_off', '<i4'), ('in_base', '<i4'), ('in_len', '<i4'), ('flags', '<i4')])


class _Axis:
    """The items of one hg_data_resample_axis launch and their concatenated tables."""

    def __init__(self, axis):
        self.axis, self.items, self.tabs, self.rows, self.ksize, self.max_bytes = axis, [], [], 0, 1, 1

    def add(self, src, src_stride, dst, dst_stride, n_keep, in_base, in_len, bounds, coeffs):
        n_out = bounds.shape[0]
        self.items.append((src, dst, src_stride, dst_stride, n_out, n_keep, self.rows, in_base, in_len, 0))
        self.tabs.append((bounds, coeffs))
        self.rows += n_out
        self.ksize = max(self.ksize, coeffs.shape[1])
        self.max_bytes = max(self.max_bytes, (3 if self.axis == 1 else 1) * n_out * n_keep)

    def tables(self):
        bounds = np.concatenate([b for b, _ in self.tabs])
        coeffs = np.zeros((self.rows, self.ksize), np.int32)
        r = 0
        for _, c in self.tabs:
            coeffs[r:r + c.shape[0], :c.shape[1]] = c
            r += c.shape[0]
        return bounds, coeffs


class DeviceBatchOps:
    """What one batch asks of the kernels of include/hg_data.h: resizes (horizontal launch, vertical launch) and the fp32
    finish, described on the host, carried to the device by ONE pinned non-blocking upload (descriptors, tables and any
    extra float32 values of the caller), then at most three launches on the current stream.  Nothing here synchronises."""

    def __init__(self, device):
        self.device, self.h, self.v, self.fin, self.tmp_bytes, self.extra = device, _Axis(1), _Axis(0), [], 0, None
        self._tmp_items = []

    def resize(self, src, src_stride, in_w, in_h, box, out_w, out_h, dst, dst_stride, window=None):
        """`Image.resize((out_w, out_h), BILINEAR, box=box)` of the (in_h, in_w) uint8 HWC image at device address src into
        dst; window (x, y, w, h): only that part of the output is computed, and dst is its first pixel."""
        l, t, r, b = box
        wx, wy, ww, wh = window if window is not None else (0, 0, out_w, out_h)
        if not (0 <= wx and 0 <= wy and ww > 0 and wh > 0 and wx + ww <= out_w and wy + wh <= out_h):
            raise ValueError(f'resize: window {window} outside a {out_w} x {out_h} output')
        if not (0 <= l < r <= in_w and 0 <= t < b <= in_h):
            raise ValueError(f'resize: box {box} outside a {in_w} x {in_h} image')
        hb, hc = (tab[wx:wx + ww] for tab in pil_bilinear_tables(in_w, l, r, out_w))
        vb, vc = (tab[wy:wy + wh] for tab in pil_bilinear_tables(in_h, t, b, out_h))
        y0, y1 = int(vb[:, 0].min()), int((vb[:, 0] + vb[:, 1]).max())     # the source rows the vertical pass reads
        rows, tmp_stride = y1 - y0, 3 * ww
        # the intermediate's address is an offset until run() allocates the batch's scratch
        self._tmp_items.append((len(self.h.items), len(self.v.items)))
        self.h.add(src + y0 * src_stride, src_stride, self.tmp_bytes, tmp_stride, rows, 0, in_w, hb, hc)
        self.v.add(self.tmp_bytes, tmp_stride, dst, dst_stride, 3 * ww, y0, rows, vb, vc)
        self.tmp_bytes += rows * tmp_stride

    def finish(self, src, src_stride, flip):
        self.fin.append((src, 0, src_stride, 0, 0, 0, 0, 0, 0, int(bool(flip))))

    def run(self, S=None, extra=None):
        """Upload and launch.  Returns (images fp32 (n, 3, S, S) or None, `extra` as a float32 device tensor or None)."""
        from ._lib import check, lib, on_device, raw_stream
        dev = self.device
        tmp = torch.empty(max(self.tmp_bytes, 1), dtype=torch.uint8, device=dev)
        base = tmp.data_ptr()
        for hi, vi in self._tmp_items:
            it = self.h.items[hi]
            self.h.items[hi] = (it[0], it[1] + base) + it[2:]
            it = self.v.items[vi]
            self.v.items[vi] = (it[0] + base,) + it[1:]
        parts, layout, off = [], {}, 0

        def put(name, arr):
            nonlocal off
            raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
            layout[name] = off
            parts.append((off, raw))
            off += (raw.size + 15) // 16 * 16

        for name, ax in (('h', self.h), ('v', self.v)):
            if ax.items:
                bounds, coeffs = ax.tables()
                put(name + '_items', np.array(ax.items, dtype=ITEM_DTYPE))
                put(name + '_bounds', bounds)
                put(name + '_coeffs', coeffs)
        if self.fin:
            put('fin', np.array(self.fin, dtype=ITEM_DTYPE))
        if extra is not None:
            put('extra', np.asarray(extra, dtype=np.float32))
        if not off:
            return None, None
        host = torch.empty(off, dtype=torch.uint8, pin_memory=True)
        hv = host.numpy()
        for o, raw in parts:
            hv[o:o + raw.size] = raw
        buf = host.to(dev, non_blocking=True)
        at = lambda name: buf.data_ptr() + layout[name]
        out = None
        with on_device(dev):
            st = raw_stream(dev)
            for name, ax in (('h', self.h), ('v', self.v)):
                if ax.items:
                    check(lib.hg_data_resample_axis(at(name + '_items'), len(ax.items), ax.axis, ax.max_bytes, at(name + '_bounds'),
                                                    at(name + '_coeffs'), ax.rows, ax.ksize, st), 'hg_data_resample_axis')
            if self.fin:
                out = torch.empty((len(self.fin), 3, S, S), dtype=torch.float32, device=dev)
                check(lib.hg_data_finish(at('fin'), len(self.fin), S, out.data_ptr(), st), 'hg_data_finish')
        ex = None
        if extra is not None:
            n = int(np.asarray(extra).size)
            ex = buf[layout['extra']:layout['extra'] + 4 * n].view(torch.float32)
        return out, ex


class ResidentFolderData(FolderData):
    """FolderData with the images kept on the device: the same constructor, item contract and plan RNG order, and for one
    seed and folder the same batches, bit for bit.

    Each file is decoded ONCE (thread pool, uint8 RGB), uploaded as uint8 HWC, and resized on the device by the stage-1
    `Resize` of `_load_rgb` (short side -> S) into a store of uint8 chunk tensors; its target histogram is taken from the same
    upload (`post.u8_hwc_to_float`, then the histogram block).  After that a batch is made without PIL and without a pixel
    crossing the bus: centre-crop items are read through a window of the stored image, random-crop items take the two-pass
    box resample from it, and one finishing launch writes fp32 CHW with the flips -- three launches at most, fed by one small
    pinned upload, with no host synchronisation.  The resample is Pillow's integer arithmetic (pil_bilinear_tables), so the
    bytes are those of the host path.

    max_store_bytes bounds the store; images that no longer fit stay on the ingest path (decode, upload, resize into a
    per-batch staging area) every time they are drawn.  chunk_bytes: the size of one store allocation.
    Counters: hits / misses (cached / computed target histograms), decodes (files opened), resident (images in the store),
    store_bytes (device memory the store's chunks take).  RGBA datasets are not served: Pillow resizes RGBA through
    premultiplied alpha, which this path does not restate -- use FolderData."""

    def __init__(self, folder, hist_block, batch_size, image_size, device, transparent=False, seed=0, test=False,
                 hist_sampling=True, workers=8, prefetch=3, cache_hists=True, max_cached=200000, hflip=False,
                 aug_prob=0.0, max_cache_bytes=2 << 30, hist_alpha_weight=False, max_store_bytes=16 << 30,
                 chunk_bytes=256 << 20):
        if transparent:
            raise ValueError('ResidentFolderData does not serve transparent=True: Pillow resizes RGBA through premultiplied '
                             'alpha, which the device path does not restate; FolderData serves RGBA datasets')
        super().__init__(folder, hist_block, batch_size, image_size, device, transparent, seed, test, hist_sampling, workers,
                         prefetch, cache_hists, max_cached, hflip, aug_prob, max_cache_bytes, hist_alpha_weight)
        self._check_device()
        self.max_store_bytes, self.chunk_bytes = int(max_store_bytes), max(1, int(chunk_bytes))
        self.chunks, self.table = [], {}           # uint8 chunk tensors; image -> (device address, H1, W1)
        self._room = 0                             # bytes left in the last chunk
        self._pending = {}                         # image -> decode in flight (shared by the prefetched plans)
        self._hist_bytes = 0                       # size of one histogram, once one has been computed
        self.decodes = self.store_bytes = 0

    def _check_device(self):
        if torch.device(self.device).type != 'cuda':
            raise RuntimeError(f'ResidentFolderData: device {self.device}; the MI355X-native path has no CPU implementation')

    @property
    def resident(self):
        return len(self.table)

    # ---- planning: one uint8 decode per file that is not on the device yet
    @staticmethod
    def _decode(path):
        from PIL import Image
        return np.array(Image.open(path).convert('RGB'), dtype=np.uint8)      # a writable copy: torch.from_numpy takes it as is

    def _decode_job(self, i):
        fut = self._pending.get(i)
        if fut is None:
            fut = self._pending[i] = self.pool.submit(self._decode, self.paths[i])
            self.decodes += 1
        return fut

    def _full_jobs(self, need):
        return {i: self._decode_job(i) for i in need}

    def _small_jobs(self, img, flips, crops):
        return [(int(i), bool(f), c, None if int(i) in self.table else self._decode_job(int(i)))
                for i, f, c in zip(img, flips, crops)]

    # ---- the store
    def _alloc(self, nbytes):
        """Device address of nbytes in the store, or None when max_store_bytes is exhausted."""
        if nbytes > self._room:
            size = max(nbytes, min(self.chunk_bytes, self.max_store_bytes - self.store_bytes))
            if self.store_bytes + size > self.max_store_bytes:
                return None
            self.chunks.append(torch.empty(size, dtype=torch.uint8, device=self.device))
            self.store_bytes += size
            self._room = size
        chunk = self.chunks[-1]
        addr = chunk.data_ptr() + chunk.numel() - self._room
        self._room -= nbytes
        return addr

    def _hist_room(self):
        return self.cache is not None and len(self.cache) < self.max_cached and \
            self.cache_bytes + self._hist_bytes <= self.max_cache_bytes

    def _ingest(self, plan):
        """First touch of the plan's images: upload, stage-1 resize into the store (or, over budget, into the batch's
        staging area), target histogram from the same upload.  Returns (staged: image -> (address, H1, W1), what keeps
        the staging area alive)."""
        from .post import u8_hwc_to_float
        jobs = dict(plan['full'])
        want_px = set()
        for i, _, _, fut in plan['small'] or ():
            if fut is not None:
                jobs[i] = fut
                want_px.add(i)
        plan['hist_ready'], staged, todo = {}, {}, []
        for i, fut in jobs.items():
            self._pending.pop(i, None)
            need_px = i in want_px and i not in self.table
            need_h = i in plan['full'] and (self.cache is None or i not in self.cache)
            store = not self.test and i not in self.table
            eager_h = self.cache is not None and i not in self.cache and self._hist_room()
            if not (need_px or need_h or store or eager_h):
                continue                                                   # an earlier batch brought it in
            arr = fut.result()
            x = torch.from_numpy(arr).pin_memory().to(self.device, non_blocking=True)
            if need_h or eager_h:
                h = self._new_hist(i, u8_hwc_to_float(x).unsqueeze(0))
                self._hist_bytes = h.numel() * h.element_size()
                plan['hist_ready'][i] = h
            if need_px or store:
                todo.append((i, x, need_px))
        if not todo:
            return staged, None
        ops, staging, keep = DeviceBatchOps(self.device), [], []
        for i, x, need_px in todo:
            h0, w0 = int(x.shape[0]), int(x.shape[1])
            w1, h1 = stage1_size(w0, h0, self.S)
            addr = self._alloc(h1 * w1 * 3)
            if addr is None:
                if not need_px:
                    continue
                staging.append((i, x, w0, h0, w1, h1))
                continue
            self.table[i] = (addr, h1, w1)
            ops.resize(x.data_ptr(), 3 * w0, w0, h0, (0, 0, w0, h0), w1, h1, addr, 3 * w1)
            keep.append(x)
        area = None
        if staging:
            area = torch.empty(sum(3 * w1 * h1 for *_, w1, h1 in staging), dtype=torch.uint8, device=self.device)
            addr = area.data_ptr()
            for i, x, w0, h0, w1, h1 in staging:
                staged[i] = (addr, h1, w1)
                ops.resize(x.data_ptr(), 3 * w0, w0, h0, (0, 0, w0, h0), w1, h1, addr, 3 * w1)
                addr += 3 * w1 * h1
                keep.append(x)
        ops.run()
        return staged, area

    def _miss(self, i, plan):
        return plan['hist_ready'][i]                                       # computed (and counted) by _ingest

    def __next__(self):
        while len(self.queue) < self.prefetch:
            self.queue.append(self._plan())
        plan = self.queue.popleft()
        staged, staging = self._ingest(plan)       # staging: held until this batch's launches are enqueued
        ops, S = DeviceBatchOps(self.device), self.S
        n_rand = sum(c is not None for _, _, c, _ in plan['small'] or ())
        crops = torch.empty((max(n_rand, 1), S, S, 3), dtype=torch.uint8, device=self.device)
        k = 0
        for i, flip, crop_seed, _ in plan['small'] or ():
            addr, h, w = staged[i] if i in staged else self.table[i]
            if crop_seed is None:
                l, t = int(round((w - S) / 2.0)), int(round((h - S) / 2.0))   # CenterCrop, as _load_rgb
                ops.finish(addr + (t * w + l) * 3, 3 * w, flip)
            else:
                l, t, cw, ch = _random_resized_crop_box(w, h, np.random.RandomState(crop_seed))
                dst = crops.data_ptr() + k * S * S * 3
                ops.resize(addr, 3 * w, w, h, (l, t, l + cw, t + ch), S, S, dst, 3 * S)
                ops.finish(dst, 3 * S, flip)
                k += 1
        images, ratio = ops.run(S, plan['ratio'] if 'h1' in plan else None)
        batch = {}
        if images is not None:
            batch['images'] = images
        batch['histograms'] = self._targets(plan, ratio)
        return batch


def save_image_grid(images, path, nrow=4, padding=2):
    """torchvision.utils.save_image restated: (N,C,H,W) in [0,1] -> one padded grid image."""
    from PIL import Image
    x = images.detach().float().clamp(0, 1).cpu()
    n, c, h, w = x.shape
    ncol = min(nrow, n)
    nr = (n + ncol - 1) // ncol
    grid = torch.zeros(c, nr * (h + padding) + padding, ncol * (w + padding) + padding)
    for k in range(n):
        r, cc = divmod(k, ncol)
        y0, x0 = padding + r * (h + padding), padding + cc * (w + padding)
        grid[:, y0:y0 + h, x0:x0 + w] = x[k]
    arr = (grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy())
    Image.fromarray(arr[..., :3] if c >= 3 else arr[..., 0]).save(path)
