#!/usr/bin/env python3
"""Golden vectors for the full-resolution post-processing (histogan_amd/post.py, include/hg_post.h) from the UNMODIFIED
utils/imresize.py, utils/pyramid_upsampling.py and utils/color_transfer_MKL.py of the reference.

    python tests/golden/make_golden_post.py      # writes tests/golden/post_*.npz (not listed in INDEX.json)

imresize and MKL are pure numpy and run as they are: those fixtures are pinned.  OpenCV is not available, so for the
pyramid a `cv2` module is put into sys.modules whose pyrDown / pyrUp / add / subtract come from tests/post_ref.py, a
restatement of OpenCV's rules: the reference's pyramid FLOW (padding, resizing, level indexing, swap, blend) runs
unmodified, its OpenCV border rules are restated and unpinned.  Images are stored as float32 (uint8 where they are
uint8 data); the resize tables as the reference's fp64 / int32.
"""
import json
import os
import sys
import types

import numpy as np

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

IMRESIZE = {   # name: (input shape, dtype, kwargs)
    'up_64_to_160x224': ((64, 64, 3), 'f', dict(output_shape=(160, 224))),
    'down_150x100_to_38x25': ((150, 100, 3), 'f', dict(output_shape=(38, 25))),
    'scalar_2p5': ((30, 20, 3), 'f', dict(scalar_scale=2.5)),
    'bilinear_40x30_to_70x50': ((40, 30, 3), 'f', dict(output_shape=(70, 50), method='bilinear')),
    'gray2d_33x47_to_64x80': ((33, 47), 'f', dict(output_shape=(64, 80))),
    'u8_60x45_to_100x90': ((60, 45, 3), 'u8', dict(output_shape=(100, 90))),
}

PYRAMID = {    # name: (reference (H, W), target side, levels, swapping_levels, blending)
    'pad_150x100_l5': ((150, 100), 64, 5, 1, False),
    'nopad_256x192_l6': ((256, 192), 64, 6, 1, False),
    'l1_96x64': ((96, 64), 64, 1, 1, False),
    's0_128x96_l4': ((128, 96), 64, 4, 0, False),
    'blend_128x96_l4': ((128, 96), 64, 4, 1, True),
}


def photo_like(rng, H, W):
    """A seeded uint8 image with smooth structure and noise (something like a photo, nothing like a constant)."""
    yy, xx = np.mgrid[0:H, 0:W] / max(H, W)
    chans = []
    for _ in range(3):
        f = rng.uniform(1, 6, 2)
        p = rng.uniform(0, 2 * np.pi, 2)
        chans.append(0.5 + 0.3 * np.sin(2 * np.pi * f[0] * yy + p[0]) * np.cos(2 * np.pi * f[1] * xx + p[1]))
    img = np.stack(chans, -1) + rng.normal(0, 0.06, (H, W, 3))
    return np.clip(np.round(img * 255), 0, 255).astype(np.uint8)


def main():
    sys.path.insert(0, ROOT)                        # histogan_amd (host tables) and tests/post_ref
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import post_ref
    cv2 = types.ModuleType('cv2')
    cv2.pyrDown, cv2.pyrUp, cv2.add, cv2.subtract = post_ref.pyrDown, post_ref.pyrUp, post_ref.add, post_ref.subtract
    sys.modules['cv2'] = cv2
    for m in [k for k in sys.modules if k == 'utils' or k.startswith('utils.')]:
        del sys.modules[m]
    # the reference's utils/ has no __init__.py: a namespace package loses to this repository's regular package
    # wherever that is on the path, so the repository root leaves sys.path once histogan_amd and post_ref are loaded
    sys.path[:] = [p for p in sys.path if os.path.abspath(p or '.') != ROOT]
    sys.path.insert(0, REF)                         # the reference's utils/ ahead of this repository's
    import torch
    import utils.color_transfer_MKL as RC
    import utils.imresize as RI
    import utils.pyramid_upsampling as RP
    assert os.path.dirname(RI.__file__) == os.path.join(REF, 'utils'), RI.__file__
    rng = np.random.default_rng(20261016)

    rec = {}
    for name, (shape, kind, kw) in IMRESIZE.items():
        x = photo_like(rng, shape[0], shape[1]) if kind == 'u8' else rng.random(shape).astype(np.float32)
        if kind == 'u8':
            x = x[..., :shape[2]]
        out = RI.imresize(x, **kw)
        method = kw.get('method', 'bicubic')
        if 'scalar_scale' in kw:
            scale = [float(kw['scalar_scale'])] * 2
            osz = RI.deriveSizeFromScale(x.shape, scale)
        else:
            scale, osz = RI.deriveScaleFromSize(x.shape, kw['output_shape']), kw['output_shape']
        kern = RI.cubic if method == 'bicubic' else RI.triangle
        for k, tag in ((0, 'h'), (1, 'w')):
            w, i = RI.contributions(x.shape[k], osz[k], scale[k], kern, 4.0)
            rec[f'{name}/w{tag}'], rec[f'{name}/i{tag}'] = np.squeeze(w, 1), np.squeeze(i, 1).astype(np.int32)
        rec[f'{name}/x'] = x
        rec[f'{name}/out'] = out if out.dtype == np.uint8 else out.astype(np.float32)
        rec[f'{name}/kwargs'] = np.array(json.dumps(kw))
    np.savez_compressed(os.path.join(HERE, 'post_imresize.npz'), **rec)

    for name, ((H, W), t, levels, s, blend) in PYRAMID.items():
        ref_u8 = photo_like(rng, H, W)
        target = (rng.random((3, t, t)) * 1.2 - 0.1).astype(np.float32)     # outside [0, 1] too: the clamp is pinned
        reference = torch.from_numpy(ref_u8).permute(2, 0, 1).float().div(255).unsqueeze(0)   # ToTensor
        tt = torch.from_numpy(target.copy()).unsqueeze(0)
        out = RP.pyramid_upsampling(tt, reference, levels=levels, swapping_levels=s, blending=blend)
        np.savez_compressed(os.path.join(HERE, f'post_pyr_{name}.npz'), target=target, reference_u8=ref_u8,
                            out=out[0].numpy().astype(np.float32),
                            kwargs=np.array(json.dumps(dict(levels=levels, swapping_levels=s, blending=blend))))

    rec = {}
    src = rng.random((150, 100, 3)).astype(np.float32)
    tgt = (0.45 + 0.2 * rng.standard_normal((64, 64, 3)) @ np.array([[1, .3, .1], [0, 1, .4], [0, 0, .8]])
           ).astype(np.float32)
    from PIL import Image
    photo = np.asarray(Image.open(os.path.join(REF, 'input_images', sorted(os.listdir(os.path.join(REF, 'input_images')))[0])).convert('RGB'))
    crop = np.ascontiguousarray(photo[:150, :100])
    for name, (s_, t_) in {'seeded_150x100_vs_64': (src, tgt),
                           'photo_crop_150x100_vs_64': ((crop / 255).astype(np.float32), tgt)}.items():
        A = np.cov(np.reshape(s_.astype(np.float64), (-1, 3), 'F'), rowvar=False)
        B = np.cov(np.reshape(t_.astype(np.float64), (-1, 3), 'F'), rowvar=False)
        rec[f'{name}/source'], rec[f'{name}/target'] = s_, t_
        rec[f'{name}/out'] = RC.color_transfer_MKL(s_.astype(np.float64), t_.astype(np.float64)).astype(np.float32)
        rec[f'{name}/T'] = RC.MKL(A, B)
        rec[f'{name}/A'], rec[f'{name}/B'] = A, B
    rec['photo_crop_150x100_vs_64/source_u8'] = crop
    np.savez_compressed(os.path.join(HERE, 'post_mkl.npz'), **rec)
    for f in sorted(os.listdir(HERE)):
        if f.startswith('post_'):
            print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == '__main__':
    main()
