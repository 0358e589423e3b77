"""Where the image-folder sources saturate: `next()` of data.FolderData (PIL on host threads, fp32 upload) against
data.ResidentFolderData (uint8 images resident on the device, crop / resize / flip / ToTensor in HIP) on one generated folder.

    python tools/data_probe.py [--files 512] [--side 1024] [--size 256] [--batch 32] [--workers 16] [--warm 40]
                               [--out profiles/data_resident.json]

Writes its own folder of smooth random JPEGs into a temporary directory (nothing outside the tree is read), then for
aug_prob 0 and 0.5 and for both sources reports
  cold   the first pass over the folder (files / batch batches from a fresh source: decodes, first histograms, ingest),
  warm   the steady state after every file has been touched: images/s over `--warm` batches (wall clock around the loop,
         ended by a device synchronise) and the host-side milliseconds one `next()` call takes (no synchronise inside).
The pools are sized by --workers (default 16, the CPUs a GPU job here is given), never by os.cpu_count().  Needs the GPU."""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def write_folder(path, files, side, workers):
    """Smooth random images (a coarse random grid up-sampled bicubically, plus a gradient): JPEG sizes like photographs'."""
    from PIL import Image

    def one(i):
        rs = np.random.RandomState(i)
        coarse = Image.fromarray((rs.rand(12, 12, 3) * 255).astype(np.uint8)).resize((side, side), Image.BICUBIC)
        arr = np.asarray(coarse, dtype=np.float32) + np.linspace(-30, 30, side, dtype=np.float32)[None, :, None]
        arr += rs.randn(side, side, 1).astype(np.float32) * 3.0
        Image.fromarray(arr.clip(0, 255).astype(np.uint8)).save(os.path.join(path, f'im{i:05d}.jpg'), quality=90)

    with ThreadPoolExecutor(max_workers=workers) as pool:
        list(pool.map(one, range(files)))


def probe(make, files, batch, warm, touched):
    import torch
    src = make()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cold_batches = -(-files // batch)
    for _ in range(cold_batches):
        next(src)
    torch.cuda.synchronize()
    cold = time.perf_counter() - t0
    extra = 0
    while not touched(src) and extra < 40 * cold_batches:            # random draws: the last files take a while to come up
        next(src)
        extra += 1
    for _ in range(src.prefetch + 2):                                # the plans made before the last first touch
        next(src)
    torch.cuda.synchronize()
    host = []
    t0 = time.perf_counter()
    for _ in range(warm):
        h0 = time.perf_counter()
        next(src)
        host.append(time.perf_counter() - h0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = dict(cold_first_pass_s=round(cold, 3), cold_images_per_s=round(cold_batches * batch / cold, 1),
               batches_until_every_file_touched=cold_batches + extra, every_file_touched=bool(touched(src)),
               warm_images_per_s=round(warm * batch / dt, 1), warm_ms_per_batch=round(1e3 * dt / warm, 3),
               warm_host_ms_per_batch_median=round(1e3 * float(np.median(host)), 3),
               warm_host_ms_per_batch_mean=round(1e3 * float(np.mean(host)), 3),
               hist_hits=src.hits, hist_misses=src.misses)
    for k in ('decodes', 'resident', 'store_bytes'):
        if hasattr(src, k):
            out[k] = int(getattr(src, k))
    src.pool.shutdown(wait=True, cancel_futures=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--files', type=int, default=512)
    ap.add_argument('--side', type=int, default=1024)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--warm', type=int, default=40)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'data_resident.json'))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('data_probe: no GPU; there is nothing to measure without one')
    from histogan_amd.data import FolderData, ResidentFolderData
    from histogram_classes.RGBuvHistBlock import RGBuvHistBlock
    dev = torch.device('cuda:0')
    blk = RGBuvHistBlock(insz=150, h=64, method='inverse-quadratic', resizing='sampling')      # the Trainer's defaults
    res = dict(tool='tools/data_probe.py', gpu=torch.cuda.get_device_name(0), files=a.files, side=a.side, image_size=a.size,
               batch=a.batch, workers=a.workers, warm_batches=a.warm, runs={})
    with tempfile.TemporaryDirectory() as folder:
        t0 = time.perf_counter()
        write_folder(folder, a.files, a.side, a.workers)
        res['folder_write_s'] = round(time.perf_counter() - t0, 2)
        res['folder_bytes'] = sum(os.path.getsize(os.path.join(folder, f)) for f in os.listdir(folder))
        kw = dict(seed=0, workers=a.workers, hflip=True)
        for aug in (0.0, 0.5):
            host = probe(lambda: FolderData(folder, blk, a.batch, a.size, dev, aug_prob=aug, **kw), a.files, a.batch, a.warm,
                         lambda s: len(s.cache) == a.files)
            dev_ = probe(lambda: ResidentFolderData(folder, blk, a.batch, a.size, dev, aug_prob=aug, **kw), a.files, a.batch,
                         a.warm, lambda s: s.resident == a.files and len(s.cache) == a.files)
            res['runs'][f'aug_prob_{aug}'] = dict(FolderData=host, ResidentFolderData=dev_,
                                                  warm_speedup=round(dev_['warm_images_per_s'] / host['warm_images_per_s'], 2))
            print(json.dumps({f'aug_prob_{aug}': res['runs'][f'aug_prob_{aug}']}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
