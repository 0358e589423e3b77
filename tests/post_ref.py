"""fp64 numpy restatement of the full-resolution post-processing (histogan_amd/post.py, include/hg_post.h), the yardstick
of the GPU tests where the reference itself is not available.

- pyrDown / pyrUp / add / subtract restate OpenCV's rules (OpenCV is not a dependency here): pyrDown filters with the
  5x5 binomial [1 4 6 4 1]^2/256 under BORDER_REFLECT_101 and keeps every second row and column; pyrUp inserts zeros
  and filters with [1 4 6 4 1]/8 per axis, its source extended by s[-1] = s[1] (reflect-101) at the left / top and
  s[n] = s[n-1] (replicate) at the right / bottom.  These border rules are restated, NOT pinned against OpenCV.
  tests/golden/make_golden_post.py runs the reference's unmodified utils/pyramid_upsampling.py with these functions in
  place of cv2, which pins the rest of its flow (padding, resizing, level indexing, swap, blend).
- imresize, pyramid_upsampling and color_transfer restate utils/imresize.py, utils/pyramid_upsampling.py and
  utils/color_transfer_MKL.py in fp64 on the host-built tables of histogan_amd.post.contributions (pinned by the
  fixtures in tests/golden/post_*.npz).
"""
import numpy as np

from histogan_amd.post import KERNEL_WIDTH, KERNELS, MKL, contributions, level_weights, padded_size, resize_plan

K5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0])


def _refl101(p, n):
    if n == 1:
        return np.zeros_like(p)
    p = np.abs(p)
    p = np.where(p >= n, 2 * n - 2 - p, p)
    return np.clip(np.abs(p), 0, n - 1)


def pyrDown(img):
    """cv2.pyrDown of an (H, W) or (H, W, C) float array, in fp64."""
    x = np.asarray(img, dtype=np.float64)
    H, W = x.shape[:2]
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    rows = [_refl101(2 * np.arange(Ho) + a - 2, H) for a in range(5)]
    cols = [_refl101(2 * np.arange(Wo) + b - 2, W) for b in range(5)]
    out = 0.0
    for a in range(5):
        xr = x[rows[a]]
        out = out + K5[a] * sum(K5[b] * xr[:, cols[b]] for b in range(5))
    return out / 256.0


def _up_axis(x, axis):
    x = np.moveaxis(x, axis, 0)
    n = x.shape[0]
    i = np.arange(n)
    prv = np.where(i > 0, i - 1, min(1, n - 1))
    nxt = np.minimum(i + 1, n - 1)
    out = np.empty((2 * n,) + x.shape[1:])
    out[0::2] = (x[prv] + 6.0 * x + x[nxt]) / 8.0
    out[1::2] = (x + x[nxt]) / 2.0
    return np.moveaxis(out, 0, axis)


def pyrUp(img):
    """cv2.pyrUp of an (H, W) or (H, W, C) float array to (2H, 2W), in fp64."""
    return _up_axis(_up_axis(np.asarray(img, dtype=np.float64), 0), 1)


def add(a, b):
    return np.asarray(a, dtype=np.float64) + b


def subtract(a, b):
    return np.asarray(a, dtype=np.float64) - b


# ---- imresize ---------------------------------------------------------------------------------------------------------
def _resize_axis(x, axis, w, idx):
    x = np.moveaxis(x, axis, 0)
    out = 0.0
    for t in range(w.shape[1]):
        out = out + w[:, t].reshape((-1,) + (1,) * (x.ndim - 1)) * x[idx[:, t]]
    return np.moveaxis(out, 0, axis)


def imresize(I, output_shape=None, scalar_scale=None, method='bicubic', with_raw=False):
    """utils/imresize.py in fp64: (H, W[, C]) array in; float64 out, or uint8 (clip + round half to even after each
    pass) for uint8 input.  with_raw: also return the unrounded fp64 value of every pass (uint8 tolerance checks)."""
    I = np.asarray(I)
    u8 = I.dtype == np.uint8
    (Ho, Wo), scale = resize_plan(I.shape[:2], output_shape, scalar_scale)
    tabs = [contributions(I.shape[k], (Ho, Wo)[k], scale[k], KERNELS[method], KERNEL_WIDTH) for k in range(2)]
    order = np.argsort(np.array(scale))
    B, raw = I, []
    for axis in order:
        v = _resize_axis(B.astype(np.float64), int(axis), *tabs[axis])
        raw.append((int(axis), v))
        B = np.around(np.clip(v, 0, 255)).astype(np.uint8) if u8 else v
    return (B, raw, tabs) if with_raw else B


def u8_near_boundary(raw, tabs, tol=5e-3):
    """Mask of uint8 imresize outputs whose value may legitimately differ by 1 LSB from an fp32 computation: the final
    fp64 value, or an intermediate one feeding it, lies within `tol` of a rounding boundary (x.5)."""
    near = lambda v: np.abs(np.abs(v - np.floor(v)) - 0.5) < tol  # noqa: E731
    (a0, v0), (a1, v1) = raw
    m0 = near(np.clip(v0, 0, 255)).astype(np.float64)
    w, idx = tabs[a1]
    feed = _resize_axis(m0, a1, (w != 0).astype(np.float64), idx) > 0
    return feed | near(np.clip(v1, 0, 255))


# ---- pyramid ------------------------------------------------------------------------------------------------------------
def gaussian_pyramid(x, n):
    g = [np.asarray(x, dtype=np.float64)]
    for _ in range(n - 1):
        g.append(pyrDown(g[-1]))
    return g


def pyramid_upsampling(target, reference, levels=5, swapping_levels=1, blending=False):
    """target (3, h, w), reference (3, H, W) float arrays -> fp64 (3, H', W') (utils/pyramid_upsampling.py)."""
    ab = level_weights(levels, swapping_levels, blending)
    t = np.clip(np.asarray(target, dtype=np.float64), 0, 1).transpose(1, 2, 0)
    r = np.asarray(reference, dtype=np.float64).transpose(1, 2, 0)
    size = padded_size(r.shape[0], r.shape[1], levels)
    if size != r.shape[:2]:
        r = imresize(r, output_shape=size)
    t = imresize(t, output_shape=size)
    ga, gb = gaussian_pyramid(t, levels), gaussian_pyramid(r, levels)
    top = levels - 1
    out = ab[0][0] * ga[top] + ab[0][1] * gb[top]
    for k in range(1, levels):
        a, b = ab[k]
        la = ga[top - k] - pyrUp(ga[top - k + 1])
        lb = gb[top - k] - pyrUp(gb[top - k + 1])
        out = pyrUp(out) + (a * la + b * lb)
    return out.transpose(2, 0, 1)


# ---- colour transfer -------------------------------------------------------------------------------------------------
def color_transfer(source, target):
    """(out (H, W, 3) fp64 in [0, 1], T) for (H, W, 3) float arrays (utils/color_transfer_MKL.py)."""
    x0 = np.asarray(source, dtype=np.float64).reshape(-1, 3)
    x1 = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    T = MKL(np.cov(x0, rowvar=False), np.cov(x1, rowvar=False))
    out = (x0 - x0.mean(0)) @ T + x1.mean(0)
    return np.clip(np.real(out), 0, 1).reshape(np.shape(source)), T


def mkl_sign_variants(A, B):
    """Every T the MKL algebra gives for the 64 sign choices of the eigenvectors of A and of C.  Because EPS is added to
    the off-diagonal entries of the eigenvalue matrices too, T depends on the signs LAPACK happens to return, at a
    relative size of about sqrt(EPS / smallest eigenvalue of A): 2.6e-5 for a near-grey photo crop whose colour
    covariance has an eigenvalue of 7.6e-6.  A last-digit change of A can flip those signs, in the reference as here."""
    from itertools import product
    from histogan_amd.post import EPS
    ea, Ua0 = np.linalg.eig(np.asarray(A, dtype=np.float64))
    out = []
    for sa in product((1.0, -1.0), repeat=3):
        Ua = Ua0 * np.array(sa)
        Da2 = np.diag(ea)
        Da2[Da2 < 0] = 0
        Da = np.sqrt(Da2 + EPS)
        ec, Uc0 = np.linalg.eig(Da @ Ua.T @ B @ Ua @ Da)
        Dc2 = np.diag(ec)
        Dc2[Dc2 < 0] = 0
        Dc = np.sqrt(Dc2 + EPS)
        Di = np.diag(1.0 / np.diag(Da))
        for sc in product((1.0, -1.0), repeat=3):
            Uc = Uc0 * np.array(sc)
            out.append(Ua @ Di @ Uc @ Dc @ Uc.T @ Di @ Ua.T)
    return out


def save_image_u8(chw):
    """torchvision save_image's quantisation of one (3, H, W) image, in fp64: (H, W, 3) uint8."""
    return np.clip(np.asarray(chw, dtype=np.float64) * 255 + 0.5, 0, 255).astype(np.uint8).transpose(1, 2, 0)
