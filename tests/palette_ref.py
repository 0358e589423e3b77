"""numpy restatement of the palette of include/hg_post.h (hg_palette_*): every integer stage in int64 (seed scores in Python
integers), the transfer in fp64 and, for the noise floor of the kernels' comparison, in fp32 arithmetic; and the seeded
inputs the tests share.  Nothing here imports the package."""
import numpy as np

UNIT = 128
SIDE, CELLS = 16, 4096
CELL_L, AB_SHIFT, AB_OFFSET = 800, 11, 16384
MAX_K = 16
NO_LABEL = 255

_M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
M = _M / _M.sum(axis=1, keepdims=True)
MI = np.linalg.inv(M)
DELTA = 6.0 / 29.0


# ---- the chain (hg_lab.h), in Lab units, unrounded --------------------------------------------------------------------
def srgb_to_lab(rgb, dtype=np.float64, root='cbrt'):
    """(..., 3) sRGB -> (..., 3) (L, a, b) in the arithmetic of `dtype`; the input is clamped to [0, 1].  root: 'cbrt' or 'pow' --
    two formulations of the same chain (the cube root as cbrt(t) or t ** (1/3), the gamma as a power or as exp(2.4 log))."""
    c = np.clip(np.asarray(rgb), 0, 1).astype(dtype)
    hi = (c + dtype(0.055)) / dtype(1.055)
    gamma = np.power(hi, dtype(2.4)) if root == 'cbrt' else np.exp(dtype(2.4) * np.log(hi))
    lin = np.where(c <= dtype(0.04045), c / dtype(12.92), gamma)
    t = lin @ M.astype(dtype).T
    big = np.cbrt(t) if root == 'cbrt' else np.power(t, dtype(1.0) / dtype(3.0))
    f = np.where(t > dtype(DELTA ** 3), big, t * dtype(1.0 / (3.0 * DELTA * DELTA)) + dtype(4.0 / 29.0))
    return np.stack([dtype(116.0) * f[..., 1] - dtype(16.0), dtype(500.0) * (f[..., 0] - f[..., 1]),
                     dtype(200.0) * (f[..., 1] - f[..., 2])], axis=-1)


def lab_to_srgb(lab, dtype=np.float64):
    """The inverse, clipped to [0, 1]."""
    lab = np.asarray(lab).astype(dtype)
    fy = (lab[..., 0] + dtype(16.0)) / dtype(116.0)
    f = np.stack([fy + lab[..., 1] / dtype(500.0), fy, fy - lab[..., 2] / dtype(200.0)], axis=-1)
    xyz = np.where(f > dtype(DELTA), f * f * f, (f - dtype(4.0 / 29.0)) * dtype(3.0 * DELTA * DELTA))
    lin = xyz @ MI.astype(dtype).T
    with np.errstate(invalid='ignore'):
        c = np.where(lin <= dtype(0.04045 / 12.92), dtype(12.92) * lin,
                     dtype(1.055) * np.power(np.maximum(lin, dtype(0)), dtype(1.0 / 2.4)) - dtype(0.055))
    return np.clip(c, dtype(0), dtype(1))


# ---- integer stages ---------------------------------------------------------------------------------------------------
def quantize(rgb, weight=None, root='cbrt'):
    """(N, 3) fp32 pixels [, (N,) fp32 weights] -> int64 (N, 4) points (qL, qa, qb, qw)."""
    rgb = np.asarray(rgb, dtype=np.float32).reshape(-1, 3)
    w = np.ones(rgb.shape[0], dtype=np.float32) if weight is None else np.asarray(weight, dtype=np.float32).reshape(-1)
    ok = np.isfinite(rgb).all(axis=1) & np.isfinite(w)
    safe = np.where(ok[:, None], rgb, np.float32(0))
    q = np.rint(UNIT * srgb_to_lab(safe, root=root)).astype(np.int64)
    qw = np.rint(65535.0 * np.clip(np.where(ok, w, np.float32(0)), 0, 1).astype(np.float64)).astype(np.int64)
    pts = np.concatenate([q, qw[:, None]], axis=1)
    pts[~ok] = 0
    return pts


def cell_of(pts):
    bL = np.minimum(np.maximum(pts[:, 0], 0) // CELL_L, SIDE - 1)
    ba = np.clip((pts[:, 1] + AB_OFFSET) >> AB_SHIFT, 0, SIDE - 1)
    bb = np.clip((pts[:, 2] + AB_OFFSET) >> AB_SHIFT, 0, SIDE - 1)
    return (bL * SIDE + ba) * SIDE + bb


def bins(pts):
    """int64 (4096, 4): W and S of every cell."""
    pts = np.asarray(pts, dtype=np.int64)
    out = np.zeros((CELLS, 4), dtype=np.int64)
    live = pts[:, 3] > 0
    c = cell_of(pts[live])
    w = pts[live, 3]
    np.add.at(out[:, 0], c, w)
    for a in range(3):
        np.add.at(out[:, 1 + a], c, w * pts[live, a])
    return out


def floor_mean(S, W):
    """floor((2 S + W) / (2 W)): numpy's // on integers is floor division."""
    return (2 * S + W) // (2 * W)


def seeds(cells, K):
    """Weighted farthest-point selection over the cells; scores are Python integers (exact)."""
    W = [int(v) for v in cells[:, 0]]
    live = [i for i in range(CELLS) if W[i] > 0]
    m = {i: tuple(int(floor_mean(int(cells[i, 1 + a]), W[i])) for a in range(3)) for i in live}
    out = np.zeros((K, 3), dtype=np.int64)
    if not live:
        return out
    first = max(live, key=lambda i: (W[i], -i))
    out[0] = m[first]
    mind = {i: sum((m[i][a] - m[first][a]) ** 2 for a in range(3)) for i in live}
    for j in range(1, K):
        best = max(live, key=lambda i: (W[i] * mind[i], -i))
        if W[best] * mind[best] == 0:
            out[j:] = out[0]
            break
        out[j] = m[best]
        for i in live:
            mind[i] = min(mind[i], sum((m[i][a] - m[best][a]) ** 2 for a in range(3)))
    return out


def distances(pts, centres):
    d = np.asarray(pts, dtype=np.int64)[:, None, :3] - np.asarray(centres, dtype=np.int64)[None, :, :]
    return (d * d).sum(axis=2)


def step(assign, value, centres):
    """(sums int64 (K, 4), labels uint8 (N,)): one Lloyd step; argmin takes the lowest index on ties."""
    assign, value = np.asarray(assign, dtype=np.int64), np.asarray(value, dtype=np.int64)
    K = len(centres)
    lab = np.argmin(distances(assign, centres), axis=1)
    live = assign[:, 3] > 0
    sums = np.zeros((K, 4), dtype=np.int64)
    w = assign[live, 3]
    np.add.at(sums[:, 0], lab[live], w)
    for a in range(3):
        np.add.at(sums[:, 1 + a], lab[live], w * value[live, a])
    return sums, np.where(live, lab, NO_LABEL).astype(np.uint8)


def update(sums, centres):
    out = np.array(centres, dtype=np.int64)
    for k in range(len(out)):
        if sums[k, 0] > 0:
            out[k] = floor_mean(sums[k, 1:], sums[k, 0])
    return out


def cost(pts, centres):
    """The integer k-means cost sum qw min_k d^2, as a Python integer."""
    pts = np.asarray(pts, dtype=np.int64)
    return int((pts[:, 3] * distances(pts, centres).min(axis=1)).sum())


def run(pts, K, iterations, value=None):
    """(centres, sums, labels, centres_other or None) of hg_palette_run on points."""
    c = seeds(bins(pts), K)
    for _ in range(iterations):
        s, _ = step(pts, pts, c)
        c = update(s, c)
    sums, labels = step(pts, pts, c)
    other = None
    if value is not None:
        s2, _ = step(pts, value, c)
        other = update(s2, c)
        c = update(sums, c)                  # both are means over the clusters of the last step
    return c, sums, labels, other


# ---- the transfer -------------------------------------------------------------------------------------------------------
def default_sigma(src, live):
    idx = [k for k in range(len(src)) if live[k]]
    d = [float(np.sqrt(((np.float64(src[i]) - np.float64(src[j])) ** 2).sum())) for n, i in enumerate(idx) for j in idx[n + 1:]]
    mean = sum(d) / len(d) if d else 0.0
    return float(np.float32(mean)) if mean > 0 else 1.0


def separating_sigma(src, live=None):
    """A quarter of the smallest distance between two live centres: a pixel on its own centre then weighs the nearest other one
    by exp(-4^2 / 2) = 3.4e-4, so well-separated colour regions move independently.  (The default sigma, the MEAN distance,
    is deliberately smooth: it weighs a centre one mean distance away by exp(-1/2).)"""
    src = np.asarray(src, dtype=np.float64)
    idx = [k for k in range(len(src)) if live is None or live[k]]
    return min(float(np.sqrt(((src[i] - src[j]) ** 2).sum())) for n, i in enumerate(idx) for j in idx[n + 1:]) / 4.0


def transfer(rgb, src, dst, live=None, sigma=None, dtype=np.float64):
    """(out (..., 3) in [0, 1] of `dtype`, sigma used).  src, dst: (K, 3) Lab units (taken as the fp32 the kernels are handed);
    all arithmetic in `dtype`."""
    shape = np.shape(rgb)
    src, dst = np.asarray(src, dtype=np.float32), np.asarray(dst, dtype=np.float32)
    live = np.ones(len(src), dtype=bool) if live is None else np.asarray(live, dtype=bool)
    sg = default_sigma(src, live) if sigma is None else float(np.float32(sigma))
    x = srgb_to_lab(np.asarray(rgb, dtype=np.float32).reshape(-1, 3), dtype=dtype)
    if live.any():
        s, shift = src[live].astype(dtype), dst[live].astype(dtype) - src[live].astype(dtype)
        diff = x[:, None, :] - s[None]
        d = (diff * diff).sum(axis=2)
        u = np.exp(-(d - d.min(axis=1, keepdims=True)) * (dtype(1.0) / (dtype(2.0) * dtype(sg) * dtype(sg))))
        x = x + (u @ shift) / u.sum(axis=1, keepdims=True)
    return lab_to_srgb(x, dtype=dtype).reshape(shape), sg


def to_u8(out):
    """(uint8)(v * 255) on the fp32 value, as the kernels quantise."""
    return (np.asarray(out).astype(np.float32) * np.float32(255.0)).astype(np.uint8)


# ---- seeded inputs ------------------------------------------------------------------------------------------------------
def clustered(K=6, per_blob=200, seed=0, spread=0.008):
    """(pixels (K per_blob, 3) fp32 in gamut, blob index (K per_blob,)): K tight Gaussian blobs around distinct vertices of
    the grid {0.15, 0.5, 0.85}^3, shuffled."""
    rs = np.random.RandomState(300 + seed)
    grid = np.array([[r, g, b] for r in (0.15, 0.5, 0.85) for g in (0.15, 0.5, 0.85) for b in (0.15, 0.5, 0.85)])
    centres = grid[rs.permutation(len(grid))[:K]]
    blob = np.repeat(np.arange(K), per_blob)
    px = centres[blob] + rs.normal(0, spread, (K * per_blob, 3))
    order = rs.permutation(len(px))
    return np.clip(px[order], 0, 1).astype(np.float32), blob[order]


def shifted(pixels, blob, K, seed=0, size=10.0):
    """`pixels` with a different Lab offset per blob (|offset| <= size per axis), back in sRGB: what an affine map cannot do."""
    rs = np.random.RandomState(400 + seed)
    off = rs.uniform(-size, size, (K, 3)) * np.array([0.6, 1.0, 1.0])
    return lab_to_srgb(srgb_to_lab(pixels) + off[blob]).astype(np.float32)


def smooth(H=40, W=52, seed=4, grid=True):
    """(H, W, 3) fp32: the sinusoid photo of tests/test_idt_gpu.py's evaluate case, on the 8-bit grid (grid=False: before
    the rounding to it -- an image ON the grid sits on the truncation's jumps when a transfer hardly moves it)."""
    rs = np.random.RandomState(seed)
    photo = np.clip(0.5 + 0.25 * np.sin(np.mgrid[0:H, 0:W][0][..., None] / 6.0 + np.arange(3)) + rs.normal(0, 0.05, (H, W, 3)), 0, 1)
    return ((np.round(photo * 255) / 255) if grid else photo).astype(np.float32)


PHOTO_HW = (41, 51)           # 2091 pixels: not a multiple of the four a lane of the transfer takes, three workgroups
TRANSFER_CASES = ('one_colour', 'default_sigma', 'explicit_sigma', 'separating', 'not_live', 'identity')


def transfer_case(name):
    """(source (H, W, 3) fp32, src lab (K, 3) fp32, dst lab, live (K,), sigma or None) of a seeded transfer case, built on
    the reference's own palette of the photo."""
    px = smooth(*PHOTO_HW, grid=False)
    K = 1 if name == 'one_colour' else 6
    c, _, _, _ = run(quantize(px.reshape(-1, 3)), K, 4)
    src = (c / UNIT).astype(np.float32)
    dst = (src + np.random.RandomState(60).uniform(-8, 8, src.shape)).astype(np.float32)
    live = np.ones(K, dtype=bool)
    sigma = {'explicit_sigma': 6.5, 'separating': separating_sigma(src) if K > 1 else None}.get(name)
    if name == 'not_live':
        live[2] = False
    if name == 'identity':
        dst = src.copy()
    return px, src, dst, live, sigma


def ties():
    """(points int64 (N, 4), centres (3, 3)): integer points equidistant from centres 0 and 1 (and farther from 2), among
    points that are not -- the lowest index must win."""
    centres = np.array([[6000, -400, 300], [6000, 400, 300], [9000, 0, -2000]], dtype=np.int64)
    rs = np.random.RandomState(7)
    n = 64
    pts = np.stack([rs.randint(5000, 7000, n), np.zeros(n, dtype=np.int64), rs.randint(-500, 500, n), rs.randint(1, 65536, n)], axis=1)
    pts[1::4, 1] = rs.randint(1, 300, len(pts[1::4]))          # nearer to centre 1
    pts[2::4, 1] = -rs.randint(1, 300, len(pts[2::4]))         # nearer to centre 0
    return pts.astype(np.int64), centres
