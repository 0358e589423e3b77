"""Device-resident image folder on the GPU: the batched resample kernels of include/hg_data.h equal Pillow byte for byte, and
data.ResidentFolderData yields FolderData's batches -- the fp32 images bit for bit, the target histograms within the
project's histogram parity bound (1e-5 max-norm-relative: the histogram kernels sum in an order the two paths need not
share) -- while every file is decoded once, the store respects its budget, and a warm batch takes at most three launches
and no host synchronisation.  S = 16, B = 5 (divides no tile size)."""
import os

import numpy as np
import pytest
import torch

from conftest import relmax

pytestmark = pytest.mark.gpu

S, B = 16, 5


@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    """The folder of tests/test_data_cpu.py (seeded PNG / JPEG files of 30-36 x 40-52 pixels and one greyscale file), plus a
    130 x 97 file (reductions of 8.1 and 6.06) and one whose short side is S already (no stage-1 resize)."""
    from PIL import Image
    path = tmp_path_factory.mktemp('resident')
    rs = np.random.RandomState(0)
    for i in range(7):
        arr = (rs.rand(30 + i, 40 + 2 * i, 3) * 255).astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(path, f'im{i}.png' if i % 2 else f'im{i}.jpg'))
    Image.fromarray((rs.rand(20, 20) * 255).astype(np.uint8)).save(os.path.join(path, 'grey.png'))
    Image.fromarray((rs.rand(130, 97, 3) * 255).astype(np.uint8)).save(os.path.join(path, 'tall.png'))
    Image.fromarray((rs.rand(S, 41, 3) * 255).astype(np.uint8)).save(os.path.join(path, 'short_is_s.png'))
    return str(path)


@pytest.fixture(scope='module')
def blk(gpu_device):
    from histogram_classes.RGBuvHistBlock import RGBuvHistBlock
    return RGBuvHistBlock(insz=32, h=16, method='inverse-quadratic', resizing='interpolation')


def _pair(folder, blk, dev, store=None, **kw):
    """(ResidentFolderData, FolderData) on the same folder with the same arguments; store: the resident source's own."""
    from histogan_amd.data import FolderData, ResidentFolderData
    return ResidentFolderData(folder, blk, B, S, dev, **kw, **(store or {})), FolderData(folder, blk, B, S, dev, **kw)


def _same(x, y):
    assert set(x) == set(y)
    if 'images' in y:
        assert x['images'].dtype == torch.float32 and x['images'].shape == y['images'].shape
        assert torch.equal(x['images'], y['images'])
    err = relmax(x['histograms'].cpu().numpy(), y['histograms'].cpu().numpy())
    assert x['histograms'].shape == y['histograms'].shape and err <= 1e-5, err


class _Launches:
    """Counts the launches of the hg_data_* entry points (each is one kernel launch)."""

    def __init__(self, monkeypatch):
        import histogan_amd._lib as L
        self.n = 0
        for name in ('hg_data_resample_axis', 'hg_data_finish'):
            fn = getattr(L.lib, name)
            monkeypatch.setattr(L.lib, name, lambda *a, _fn=fn: self._call(_fn, a))

    def _call(self, fn, a):
        self.n += 1
        return fn(*a)


# ---- the kernels against Pillow ----------------------------------------------------------------------------------------
def test_batched_resample_equals_pillow(gpu_device, monkeypatch):
    from PIL import Image
    from histogan_amd.data import DeviceBatchOps
    rs = np.random.RandomState(1)
    shapes = [(5, 7), (37, 33), (21, 130), (9, 9), (16, 16), (40, 31), (130, 97)]          # (h, w): odd widths, unaligned rows
    imgs = [(rs.rand(h, w, 3) * 255).astype(np.uint8) for h, w in shapes]
    # the images back to back behind one odd byte, as the store packs them: no row or base is 4-byte aligned by design
    store = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8)] + [i.reshape(-1) for i in imgs])).to(gpu_device)
    addr, off = [], 1
    for i in imgs:
        addr.append(store.data_ptr() + off)
        off += i.size
    # (image, box or None, (out_w, out_h), output window (x, y, w, h) or None)
    cases = [(0, None, (16, 16), None),                          # 5 x 7: up-scale on both axes
             (1, None, (16, 16), None),                          # 37 -> 16 and 33 -> 16
             (1, None, (16, 16), (3, 2, 9, 11)),                 # ... an output window of it
             (2, None, (16, 16), None),                          # 130 -> 16 (19 taps) next to 21 -> 16
             (2, None, (99, 16), (40, 0, 16, 16)),               # a centre window of a stage-1 resize
             (3, None, (16, 16), None),                          # 9 -> 16 up-scale
             (4, None, (16, 16), None),                          # identity on both axes
             (5, (3, 5, 30, 33), (16, 16), None),                # integer box
             (5, (0, 0, 31, 17), (16, 16), (0, 0, 16, 5)),       # box at two borders, window
             (5, (2.25, 1.5, 30.75, 39.125), (23, 11), None),    # fractional box, outputs no multiple of anything
             (6, None, (16, 21), None),                          # 97 -> 16 and 130 -> 21: the tall file's stage 1
             (6, (40, 60, 97, 130), (16, 16), (5, 0, 11, 16))]   # box at the other two borders, window
    ops, outs = DeviceBatchOps(gpu_device), []
    for k, box, (ow, oh), win in cases:
        h, w = shapes[k]
        ww, wh = (win[2], win[3]) if win else (ow, oh)
        out = torch.full((wh * ww * 3 + 2,), 77, dtype=torch.uint8, device=gpu_device)    # a guard byte on each side
        outs.append(out)
        ops.resize(addr[k], 3 * w, w, h, box or (0, 0, w, h), ow, oh, out.data_ptr() + 1, 3 * ww, win)
    count = _Launches(monkeypatch)
    ops.run()
    assert count.n == 2                                           # one launch per axis for the twelve items
    for (k, box, size, win), out in zip(cases, outs):
        want = np.asarray(Image.fromarray(imgs[k]).resize(size, Image.BILINEAR, box=box))
        if win:
            want = want[win[1]:win[1] + win[3], win[0]:win[0] + win[2]]
        got = out.cpu()
        assert got[0] == 77 and got[-1] == 77, (k, box, size, win)
        assert torch.equal(got[1:-1].view(want.shape), torch.from_numpy(want.copy())), (k, box, size, win)


def test_finish_windows_flips_and_divides(gpu_device):
    from histogan_amd.data import DeviceBatchOps
    rs = np.random.RandomState(2)
    img = (rs.rand(23, 37, 3) * 255).astype(np.uint8)
    img[0, :86 // 3 + 1].reshape(-1)[:86] = np.arange(170, 256)                  # every byte value appears
    img[1].reshape(-1)[:111] = np.arange(111)
    img[2].reshape(-1)[:59] = np.arange(111, 170)
    dev_img = torch.from_numpy(img).to(gpu_device)
    ops = DeviceBatchOps(gpu_device)
    wins = [(0, 0, False), (21, 7, True), (5, 3, False), (2, 0, True), (9, 6, True)]      # (left, top, flip); B = 5 items
    for l, t, flip in wins:
        ops.finish(dev_img.data_ptr() + (t * 37 + l) * 3, 3 * 37, flip)
    out, _ = ops.run(S)
    assert out.shape == (5, 3, S, S)
    for k, (l, t, flip) in enumerate(wins):
        want = img[t:t + S, l:l + S].astype(np.float32) / 255.0                  # ToTensor, as _load_rgb
        want = want[:, ::-1] if flip else want
        assert torch.equal(out[k].cpu(), torch.from_numpy(np.ascontiguousarray(want)).permute(2, 0, 1))


# ---- source against source ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('aug_prob', [0.0, 1.0, 0.5])
def test_batches_equal_folder_data(folder, blk, gpu_device, aug_prob):
    res, ref = _pair(folder, blk, gpu_device, seed=3, hflip=True, aug_prob=aug_prob)
    for _ in range(6):
        x, y = next(res), next(ref)
        assert x['images'].shape == (B, 3, S, S) and x['images'].is_cuda
        _same(x, y)


def test_every_file_is_decoded_once_and_warm_batches_touch_no_file(folder, blk, gpu_device, monkeypatch):
    from histogan_amd.data import ResidentFolderData
    res, ref = _pair(folder, blk, gpu_device, seed=4, hflip=True, aug_prob=0.5)
    n = len(res.paths)
    assert n == 10
    for _ in range(40):                                    # until the prefetched plans hold no first touch any more
        _same(next(res), next(ref))
        if res.resident == n and len(res.cache) == n and not res._pending:
            break
    assert res.resident == n and res.decodes == n and res.misses == n
    assert 0 < res.store_bytes <= res.max_store_bytes
    for _ in range(res.prefetch):                          # the plans made before the last first touch are used up
        _same(next(res), next(ref))
    # warm: no file is opened, three launches at most, nothing synchronises the host
    monkeypatch.setattr(ResidentFolderData, '_decode', staticmethod(lambda path: pytest.fail(f'decoded {path}')))
    count = _Launches(monkeypatch)
    torch.cuda.synchronize()
    warm = []
    torch.cuda.set_sync_debug_mode('error')
    try:
        for _ in range(4):
            before = count.n
            warm.append(next(res))
            assert count.n - before <= 3
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for x in warm:
        _same(x, next(ref))
    assert res.decodes == n and res.resident == n and res.misses == n


def test_over_budget_images_stay_on_the_ingest_path(folder, blk, gpu_device):
    from PIL import Image
    from histogan_amd.data import stage1_size
    sizes = [3 * int(np.prod(stage1_size(*Image.open(os.path.join(folder, f)).size, S))) for f in sorted(os.listdir(folder))]
    budget = sum(sizes) // 2
    # chunks of 1 KiB: about one image each, so the budget is reached through several allocations
    res, ref = _pair(folder, blk, gpu_device, store=dict(max_store_bytes=budget, chunk_bytes=1 << 10), seed=5, hflip=True,
                     aug_prob=0.5, prefetch=1)
    n, plans, make = len(res.paths), [], res._plan
    res._plan = lambda: plans.append(make()) or plans[-1]
    for _ in range(12):
        resident, cached, decodes = set(res.table), set(res.cache), res.decodes
        _same(next(res), next(ref))
        plan = plans[-1]                                    # prefetch = 1: made and used by this call
        touched = {i for i, _, _, _ in plan['small'] if i not in resident} | {i for i in plan['full'] if i not in cached}
        assert res.decodes - decodes == len(touched)        # a decode per image that was not on the device, and no other
        assert res.store_bytes <= budget
    assert 0 < res.resident < n and res.store_bytes <= budget and res.decodes > n


def test_modes(folder, blk, gpu_device):
    res, ref = _pair(folder, blk, gpu_device, seed=6, test=True)
    for _ in range(2):
        x, y = next(res), next(ref)
        assert set(x) == {'histograms'}
        _same(x, y)
    assert res.resident == 0 and res.store_bytes == 0       # test mode draws no pixels: nothing is stored
    res, ref = _pair(folder, blk, gpu_device, seed=7, hist_sampling=False, hflip=True, aug_prob=0.5)
    for _ in range(3):
        _same(next(res), next(ref))
    res, ref = _pair(folder, blk, gpu_device, seed=8, cache_hists=False)
    for _ in range(2):
        _same(next(res), next(ref))


def test_trainer_keyword_selects_the_resident_source(folder, gpu_device, tmp_path):
    from histoGAN import Trainer
    from histogan_amd.data import FolderData, ResidentFolderData
    tr = Trainer('res', str(tmp_path / 'results'), str(tmp_path / 'models'), 32, 2, batch_size=2, hist_bin=16, hist_insz=32,
                 hist_resizing='interpolation', save_every=1000, aug_prob=0.0, dataset_aug_prob=0.5)
    tr.run_evaluate = tr.run_save = False
    tr.set_data_src(folder)
    assert type(tr.loader) is FolderData
    want = next(tr.loader)
    tr.set_data_src(folder, resident=True)
    assert type(tr.loader) is ResidentFolderData and type(tr.loader_evaluate) is FolderData
    got = next(tr.loader)
    assert got['images'].shape == (2, 3, 32, 32)
    _same(got, want)
    tr.train(alpha=2)
    assert tr.steps == 1 and np.isfinite(tr.d_loss) and np.isfinite(tr.g_loss)
