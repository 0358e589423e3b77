"""Pillow's 8-bit bilinear resize restated in numpy (a helper of the resident-data tests, not a test): the coefficient tables of
one axis, written as the plain loops of the definition, and the two integer passes that apply them.

    out = clip((2^21 + sum_t k[t] * pix[first + t]) >> 22, 0, 255)        per output, int32

The horizontal pass runs first, over the source rows the vertical pass reads, and its result is rounded to uint8 before the
vertical pass runs on it with its first rows rebased."""
import math

import numpy as np

BITS = 22


def tables(in_size, in0, in1, out_size):
    """(bounds int32 (out_size, 2) = (first, taps), coeffs int32 (out_size, ksize)) of one axis; fp64 as Python floats."""
    in0, in1 = np.float32(in0), np.float32(in1)              # the C entry point takes the box as four floats ...
    scale = float(in1 - in0) / out_size                      # ... and subtracts them as floats; fp64 from here on
    in0 = float(in0)
    filterscale = max(scale, 1.0)
    support = filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(in_size, int(center + support + 0.5)) - xmin
        w = [0.0] * ksize
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) / filterscale)
            w[x] = 1.0 - a if a < 1.0 else 0.0
        ww = sum(w[:xmax])                                   # left to right, as the C loop adds them
        if ww != 0.0:
            w = [v / ww if x < xmax else 0.0 for x, v in enumerate(w)]
        bounds[xx] = (xmin, xmax)
        coeffs[xx] = [int(0.5 + v * (1 << BITS)) for v in w]
    return bounds, coeffs


def apply_axis(img, bounds, coeffs, axis, base=0):
    """One pass over a uint8 (H, W, C) image; axis 1: horizontal, 0: vertical.  base: the input index of img's first
    row / column along the axis (an intermediate that holds only part of the rows)."""
    x = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.zeros((bounds.shape[0],) + x.shape[1:], np.int64)
    for o, (first, taps) in enumerate(bounds):
        acc = np.full(x.shape[1:], 1 << (BITS - 1), np.int64)
        for t in range(int(taps)):
            acc = acc + int(coeffs[o, t]) * x[int(first) - base + t]
        assert np.abs(acc).max() < 2 ** 31                  # the kernel's accumulator is int32
        out[o] = np.clip(acc >> BITS, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def resize(img, size, box=None, window=None, tables_fn=tables):
    """`Image.fromarray(img).resize(size, Image.BILINEAR, box=box)` as an array; size (w, h), box (l, t, r, b), window
    (x, y, w, h): only that part of the output."""
    H, W = img.shape[:2]
    ow, oh = size
    l, t, r, b = box if box is not None else (0, 0, W, H)
    wx, wy, ww, wh = window if window is not None else (0, 0, ow, oh)
    hb, hc = (np.asarray(v)[wx:wx + ww] for v in tables_fn(W, l, r, ow))
    vb, vc = (np.asarray(v)[wy:wy + wh] for v in tables_fn(H, t, b, oh))
    y0, y1 = int(vb[:, 0].min()), int((vb[:, 0] + vb[:, 1]).max())
    mid = apply_axis(img[y0:y1], hb, hc, 1)
    return apply_axis(mid, vb, vc, 0, base=y0)
