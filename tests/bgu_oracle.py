"""fp64 restatement of bilateral guided upsampling (the reference's upsampling/BGU.m -> bguFit.m -> bguSlice.m), numpy
only, written from the mathematics and sharing no structure with histogan_amd/post.py: the stacked least-squares system
[sqrt(W) A; R] gamma = [sqrt(W) out; 0] is built densely, row by row, and solved with np.linalg.lstsq (QR / SVD), never
through the normal equations.  Images are (H, W, 3) float64 in [0, 1]; gamma is (gh, gw, gd, 3, 4).

Unknown order of one output channel ("natural"): col = ((y * gw + x) * gd + z) * 4 + j."""
import numpy as np

GD = 8


def grid_size(h, w):
    """MATLAB round (half away from zero) of the side over 16."""
    r = lambda v: int(np.floor(v / 16 + 0.5))  # noqa: E731
    return r(h), r(w)


def luminance(img):
    return 0.25 * img[..., 0] + 0.5 * img[..., 1] + 0.25 * img[..., 2]


def _coords(img, gh, gw, gd):
    H, W = img.shape[:2]
    cy = (np.arange(H, dtype=np.float64)[:, None] + 0.5) * (gh - 1) / H + np.zeros((1, W))
    cx = (np.arange(W, dtype=np.float64)[None, :] + 0.5) * (gw - 1) / W + np.zeros((H, 1))
    cz = luminance(img) * (gd - 1)
    return cy, cx, cz


def _vertices(img, gh, gw, gd):
    """For every pixel (flattened row-major) its 8 vertices: lists of (y, x, z, weight, inside)."""
    cy, cx, cz = (c.reshape(-1) for c in _coords(img, gh, gw, gd))
    y0, x0, z0 = np.floor(cy).astype(int), np.floor(cx).astype(int), np.floor(cz).astype(int)
    fy, fx, fz = cy - y0, cx - x0, cz - z0
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            for dz in (0, 1):
                wt = (fy if dy else 1 - fy) * (fx if dx else 1 - fx) * (fz if dz else 1 - fz)
                y, x, z = y0 + dy, x0 + dx, z0 + dz
                ok = (y >= 0) & (y < gh) & (x >= 0) & (x < gw) & (z >= 0) & (z < gd)      # outside the grid: dropped
                out.append((y, x, z, wt, ok))
    return out


def data_rows(in_img, grid, gd=GD):
    """A (h*w, n): row p holds sum_v tri_v [r g b 1]_j at column (v, j); one output channel's data term, unweighted."""
    gh, gw = grid
    h, w = in_img.shape[:2]
    n = gh * gw * gd * 4
    A = np.zeros((h * w, n))
    rows = np.arange(h * w)
    feat = np.concatenate([in_img.reshape(-1, 3).astype(np.float64), np.ones((h * w, 1))], axis=1)
    for y, x, z, wt, ok in _vertices(in_img, gh, gw, gd):
        base = ((y * gw + x) * gd + z) * 4
        for j in range(4):
            np.add.at(A, (rows[ok], base[ok] + j), (wt * feat[:, j])[ok])
    return A


def smooth_rows(h, w, grid, gd=GD, lambda_spatial=1.0, lambda_z=4e-7):
    """R (rows, n): first differences in y and x, second differences in z with first differences at both ends."""
    gh, gw = grid
    n = gh * gw * gd * 4
    col = lambda y, x, z, j: ((y * gw + x) * gd + z) * 4 + j  # noqa: E731
    bx, by, bz = w / gw, h / gh, 1 / gd
    ky, kx = (bx * bz / by) * lambda_spatial, (by * bz / bx) * lambda_spatial
    kz = (bx * by / (bz * bz)) * lambda_z
    rows = []

    def row(entries, k):
        r = np.zeros(n)
        for c, v in entries:
            r[c] += k * v
        rows.append(r)

    for j in range(4):
        for z in range(gd):
            for y in range(gh):
                for x in range(gw):
                    if y + 1 < gh:
                        row([(col(y + 1, x, z, j), 1), (col(y, x, z, j), -1)], ky)
                    if x + 1 < gw:
                        row([(col(y, x + 1, z, j), 1), (col(y, x, z, j), -1)], kx)
                    if z + 2 < gd:
                        row([(col(y, x, z, j), 1), (col(y, x, z + 1, j), -2), (col(y, x, z + 2, j), 1)], kz)
                    if z == 0:
                        row([(col(y, x, 1, j), 1), (col(y, x, 0, j), -1)], kz)
                    if z == gd - 1:
                        row([(col(y, x, gd - 2, j), 1), (col(y, x, gd - 1, j), -1)], kz)
    return np.stack(rows)


def slab_permutation(grid, gd=GD):
    """perm with perm[(s * T + t) * gd * 4 + z * 4 + j] = natural column: slabs along the longer spatial axis (y when
    gh >= gw)."""
    gh, gw = grid
    perm = []
    if gh >= gw:
        for s in range(gh):
            for t in range(gw):
                perm += [((s * gw + t) * gd + z) * 4 + j for z in range(gd) for j in range(4)]
    else:
        for s in range(gw):
            for t in range(gh):
                perm += [((t * gw + s) * gd + z) * 4 + j for z in range(gd) for j in range(4)]
    return np.array(perm)


def slab_blocks(N, grid, gd=GD):
    """(diag (S, m, m), off (S - 1, m, m)) of a natural-order (n, n) matrix, off[s] = N[slab s + 1, slab s]; also
    returns the largest entry outside the block tridiagonal."""
    gh, gw = grid
    S, m = max(gh, gw), min(gh, gw) * gd * 4
    p = slab_permutation(grid, gd)
    Ns = N[np.ix_(p, p)].copy()
    diag = np.stack([Ns[s * m:(s + 1) * m, s * m:(s + 1) * m] for s in range(S)])
    off = np.stack([Ns[(s + 1) * m:(s + 2) * m, s * m:(s + 1) * m] for s in range(S - 1)])
    for s in range(S):
        Ns[s * m:(s + 1) * m, max(0, s - 1) * m:(s + 2) * m] = 0
    return diag, off, float(np.max(np.abs(Ns)))


def fit(in_img, out_img, weight=None, lambda_spatial=1.0, lambda_z=4e-7, gd=GD):
    h, w = in_img.shape[:2]
    grid = grid_size(h, w)
    A = data_rows(in_img, grid, gd)
    sw = np.sqrt(np.ones(h * w) if weight is None else np.asarray(weight, dtype=np.float64).reshape(-1))
    R = smooth_rows(h, w, grid, gd, lambda_spatial, lambda_z)
    lhs = np.concatenate([sw[:, None] * A, R])
    rhs = np.concatenate([sw[:, None] * out_img.reshape(-1, 3).astype(np.float64), np.zeros((R.shape[0], 3))])
    sol = np.linalg.lstsq(lhs, rhs, rcond=None)[0]                    # (n, 3)
    return sol.reshape(grid[0], grid[1], gd, 4, 3).transpose(0, 1, 2, 4, 3)


def slice_(gamma, img):
    """(H, W, 3) float64, not clipped.  A vertex outside the grid contributes nothing (at luminance 1 its weight is 0;
    MATLAB's interp3 would return NaN beyond that)."""
    gh, gw, gd = gamma.shape[:3]
    H, W = img.shape[:2]
    model = np.zeros((H * W, 3, 4))
    for y, x, z, wt, ok in _vertices(img, gh, gw, gd):
        model[ok] += wt[ok, None, None] * gamma[y[ok], x[ok], z[ok]]
    feat = np.concatenate([img.reshape(-1, 3).astype(np.float64), np.ones((H * W, 1))], axis=1)
    return np.einsum('pij,pj->pi', model, feat).reshape(H, W, 3)


def quantize(v):
    """MATLAB imwrite of a double image: round(255 clip(v, 0, 1)), half away from zero; also the unrounded 255 v."""
    raw = 255 * np.clip(v, 0, 1)
    return np.floor(raw + 0.5).astype(np.uint8), raw


def upsample(target_chw, photo_u8, weight=None, max_side=300):
    """BGU.m: (sliced (H, W, 3) float64, gamma).  target_chw: float (3, h, w), quantised as save_image writes it."""
    import post_ref
    out_ds = post_ref.save_image_u8(target_chw).astype(np.float64) / 255
    if out_ds.shape[0] > max_side or out_ds.shape[1] > max_side:
        out_ds = post_ref.imresize(out_ds, output_shape=(max_side, max_side))
    photo = photo_u8.astype(np.float64) / 255
    in_ds = post_ref.imresize(photo, output_shape=out_ds.shape[:2])
    gamma = fit(in_ds, out_ds, weight)
    return slice_(gamma, photo), gamma


# ---- the synthetic cases the tests share ------------------------------------------------------------------------------
def synthetic_photo(seed, H, W):
    """uint8 (H, W, 3): smooth colour waves plus noise, with one pure black and one pure white block (luminance 0 and
    1: the latter is the dropped-vertex case)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W] / max(H, W)
    ch = [0.5 + 0.3 * np.sin(2 * np.pi * rng.uniform(1, 4) * yy + rng.uniform(0, 6)) *
          np.cos(2 * np.pi * rng.uniform(1, 4) * xx + rng.uniform(0, 6)) for _ in range(3)]
    img = np.clip(np.round((np.stack(ch, -1) + rng.normal(0, 0.04, (H, W, 3))) * 255), 0, 255).astype(np.uint8)
    img[H // 8:H // 8 + max(2, H // 10), W // 6:W // 6 + max(2, W // 8)] = 0
    img[H // 2:H // 2 + max(2, H // 10), W // 2:W // 2 + max(2, W // 8)] = 255
    return img


def recolour(img):
    """A smooth global recolouring of an (h, w, 3) image in [0, 1]: a tone curve and a channel mix."""
    M = np.array([[0.70, 0.25, 0.05], [0.10, 0.65, 0.20], [0.15, 0.05, 0.85]])
    return np.clip(np.clip(img, 0, 1) ** 0.8 @ M.T * 0.9 + np.array([0.04, 0.02, 0.06]), 0, 1)


def synthetic_target(photo_u8, h, w):
    """float32 (3, h, w): the recoloured low-resolution photo on exact 8-bit levels k / 255, so that save_image's
    quantisation returns k whatever the precision it is evaluated in."""
    import post_ref
    low = post_ref.imresize(photo_u8.astype(np.float64) / 255, output_shape=(h, w))
    k = np.floor(255 * recolour(low) + 0.5)
    return (k / 255).astype(np.float32).transpose(2, 0, 1).copy()


def excused(raw, delta=0.01):
    """Values whose unrounded 255 v lies within delta of a rounding boundary (k + 0.5)."""
    return np.abs(raw - np.floor(raw) - 0.5) < delta


_LOWRES = {}


def lowres_case(h, w):
    """(in_ds, out_ds, weight) float32 (h, w, 3) / (h, w) at low resolution, computed once: the fp64 resize of a
    synthetic photo with black and white blocks, its recolouring, and a weight map with a zero region."""
    if (h, w) not in _LOWRES:
        import post_ref
        photo = synthetic_photo(5, 2 * h + 3, 2 * w + 1)
        in_ds = post_ref.imresize(photo.astype(np.float64) / 255, output_shape=(h, w)).astype(np.float32)
        in_ds[h // 8:h // 8 + 3, w // 6:w // 6 + 3] = 0            # the resize blurs the blocks: keep luminance 0 and 1
        in_ds[h // 2:h // 2 + 3, w // 2:w // 2 + 3] = 1
        out_ds = synthetic_target(photo, h, w).transpose(1, 2, 0).copy()
        wt = np.random.default_rng(h).uniform(0.2, 2.0, (h, w)).astype(np.float32)
        wt[h // 3:h // 3 + 9, : w // 2] = 0
        _LOWRES[(h, w)] = (in_ds, out_ds, wt)
    return _LOWRES[(h, w)]


LOWRES_SHAPES = [(64, 48), (40, 72), (50, 35)]      # grids (4, 3), (3, 5), (3, 2): both slab orientations, unequal cells
PLAIN_ATA_ERR = 8.52e-16        # numpy's fp64 A^T W A against long double, fraction of the largest entry, worst case
PLAIN_ATB_ERR = 7.3e-16         # ... and A^T W out


def normal_long_double(A, wv, out):
    """(A^T W A, A^T W out) in long double, using that a row of A has at most 32 non-zeros."""
    k = min(32, A.shape[1])
    idx = np.argsort(-np.abs(A), axis=1, kind='stable')[:, :k]
    assert np.count_nonzero(A) == np.count_nonzero(np.take_along_axis(A, idx, 1))
    v = np.take_along_axis(A, idx, 1).astype(np.longdouble)
    wl = wv.astype(np.longdouble)[:, None]
    N = np.zeros((A.shape[1], A.shape[1]), dtype=np.longdouble)
    np.add.at(N, (idx[:, :, None], idx[:, None, :]), (wl * v)[:, :, None] * v[:, None, :])
    b = np.zeros((A.shape[1], out.shape[1]), dtype=np.longdouble)
    np.add.at(b, idx, ((wl * v)[:, :, None] * out.astype(np.longdouble)[:, None, :]))
    return N, b
