"""numpy restatement of include/hg_lut.h: 3D colour LUTs in fp64 and integers.

apply     the interpolants of hg_lut_apply; dtype=np.float32 evaluates the same formula in fp32 arithmetic (its distance to the
          fp64 evaluation is the eps32 the GPU tests take their bar from).
splat     the integer normal sums of hg_lut_splat, exactly.
solve     the red-black Gauss-Seidel sequence of hg_lut_solve, update for update (numpy contracts nothing into fma either).
direct    the same system through scipy's sparse LU: what the sweeps converge to.
synthetic a smooth random colour image and a smooth, non-affine colour map of it: the pair the fit is judged on.
"""
import numpy as np

FB, WB, DB = 5, 8, 16                 # HG_LUT_COORD_BITS, HG_LUT_WEIGHT_BITS, HG_LUT_DISP_BITS
ONE = 1 << FB
MAX_N, MAX_PIXELS = 65, 1 << 22
DEFAULT_LAMBDA, DEFAULT_SWEEPS = 0.2, 128       # post.LUT_LAMBDA, post.LUT_SWEEPS


def identity(n):
    g = np.arange(n, dtype=np.float64) / (n - 1)
    lut = np.empty((n, n, n, 3))
    lut[..., 0], lut[..., 1], lut[..., 2] = g[None, None, :], g[None, :, None], g[:, None, None]
    return lut


def clamp01(x):
    """fminf(fmaxf(x, 0), 1) on fp32: NaN reads as 0."""
    return np.fmin(np.fmax(np.asarray(x, dtype=np.float32), np.float32(0)), np.float32(1))


def levels(v_u8):
    """The fp32 value a uint8 source level reads as."""
    return np.asarray(v_u8).astype(np.float32) / np.float32(255)


def fma32(a, b, c):
    """fmaf(a, b, c) of fp32 scalars: the exact a b + c (rationals) rounded once to fp32, ties to even."""
    from fractions import Fraction
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    near = np.float32(float(exact))
    cands = [np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf))]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))


def level_without_division(v):
    """The kernel's sequence for a uint8 level: q = v r, then fmaf(fmaf(-q, 255, v), r, q), r = fl(1 / 255)."""
    r = np.float32(1) / np.float32(255)
    q = np.float32(v) * r
    return fma32(fma32(-q, np.float32(255), np.float32(v)), r, q)


def cell(x, n, dtype=np.float64):
    """(i, f) of fp32 pixels x (M, 3): i from the fp32 product, f = fma(x, n - 1, -i) (the exact difference, rounded once)."""
    xc = clamp01(x)
    i = np.minimum((xc * np.float32(n - 1)).astype(np.int64), n - 2)
    f = xc.astype(np.float64) * (n - 1) - i
    return i, f.astype(np.float32).astype(dtype) if dtype == np.float32 else f


def apply(x, lut, interpolation='tetrahedral', dtype=np.float64):
    """x: (M, 3) fp32; lut: (n, n, n, 3).  The clipped output (M, 3) in `dtype` arithmetic."""
    n = lut.shape[0]
    L = np.asarray(lut).astype(dtype)
    i, f = cell(x, n, dtype)
    M = len(i)
    at = lambda idx: L[idx[:, 2], idx[:, 1], idx[:, 0]]
    if interpolation == 'tetrahedral':
        order = np.argsort(-f, axis=1, kind='stable')
        idx = i.copy()
        v = at(idx)
        out = v
        for k in range(3):
            ax = order[:, k]
            idx[np.arange(M), ax] += 1
            nxt = at(idx)
            out = out + f[np.arange(M), ax][:, None] * (nxt - v)
            v = nxt
    elif interpolation == 'trilinear':
        def corner(jr, jg, jb):
            return at(i + np.array([jr, jg, jb]))
        lerp = lambda u, v, t: u + t[:, None] * (v - u)
        e = [[lerp(corner(0, jg, jb), corner(1, jg, jb), f[:, 0]) for jg in (0, 1)] for jb in (0, 1)]
        out = lerp(lerp(e[0][0], e[0][1], f[:, 1]), lerp(e[1][0], e[1][1], f[:, 1]), f[:, 2])
    else:
        raise ValueError(interpolation)
    return np.minimum(np.maximum(out, dtype(0)), dtype(1))


def quantize(out):
    """(uint8)(v * 255): truncation."""
    return (out * out.dtype.type(255)).astype(np.uint8)


# ---- fit ---------------------------------------------------------------------------------------------------------------
def fixed_point(s, t, w, n):
    """(i (M, 3), f (M, 3) in [0, 32], qd (M, 3), qw (M,)) of fp32 pixel pairs: int64."""
    s, t = np.asarray(s, dtype=np.float32).reshape(-1, 3), np.asarray(t, dtype=np.float32).reshape(-1, 3)
    wv = np.ones(len(s), dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32).reshape(-1)
    ok = np.isfinite(s).all(1) & np.isfinite(t).all(1) & np.isfinite(wv)
    s, t, wv = np.where(ok[:, None], s, 0).astype(np.float32), np.where(ok[:, None], t, 0).astype(np.float32), np.where(ok, wv, 0)
    qw = np.rint(clamp01(wv).astype(np.float64) * (1 << WB)).astype(np.int64)
    xc = clamp01(s).astype(np.float64)
    q = np.rint(xc * ((n - 1) << FB)).astype(np.int64)
    i = np.minimum(q >> FB, n - 2)
    f = q - (i << FB)
    qd = np.rint(np.clip(t.astype(np.float64) - xc, -2.0, 2.0) * (1 << DB)).astype(np.int64)
    return i, f, qd, qw


def splat(s, t, w, n):
    """sums int64 (n, n, n, 4) = (A, B_r, B_g, B_b), indexed [ib, ig, ir]."""
    i, f, qd, qw = fixed_point(s, t, w, n)
    sums = np.zeros((n * n * n, 4), dtype=np.int64)
    for j in range(8):
        jr, jg, jb = j & 1, (j >> 1) & 1, j >> 2
        om = (f[:, 0] if jr else ONE - f[:, 0]) * (f[:, 1] if jg else ONE - f[:, 1]) * (f[:, 2] if jb else ONE - f[:, 2])
        wa = qw * om
        keep = wa != 0
        node = ((i[:, 2] + jb) * n + i[:, 1] + jg) * n + i[:, 0] + jr
        np.add.at(sums[:, 0], node[keep], wa[keep])
        for c in range(3):
            np.add.at(sums[:, 1 + c], node[keep], (wa * qd[:, c])[keep])
    return sums.reshape(n, n, n, 4)


def degree(n):
    e = np.full(n, 2.0)
    e[0] = e[-1] = 1.0
    return e[:, None, None] + e[None, :, None] + e[None, None, :]


def system(sums, n, c):
    """(a, b) (n, n, n) fp64 of channel c, or None when there is no data at all."""
    S = int(sums[..., 0].sum())
    if S == 0:
        return None
    scale = float(n ** 3) / float(S)
    return sums[..., 0].astype(np.float64) * scale, (sums[..., 1 + c].astype(np.float64) * scale) * (1.0 / (1 << DB))


def neighbour_sum(d):
    """Sum over the existing neighbours in the order r - 1, r + 1, g - 1, g + 1, b - 1, b + 1 (axes: [ib, ig, ir])."""
    z = np.zeros_like(d)
    nb = z.copy()
    for ax in (2, 1, 0):
        lo, hi = z.copy(), z.copy()
        sl = [slice(None)] * 3
        a, b = list(sl), list(sl)
        a[ax], b[ax] = slice(1, None), slice(None, -1)
        lo[tuple(a)] = d[tuple(b)]           # the neighbour at index - 1
        hi[tuple(b)] = d[tuple(a)]           # the neighbour at index + 1
        nb = (nb + lo) + hi
    return nb


def solve_channel(a, b, lam, sweeps, history=None):
    n = a.shape[0]
    den = a + lam * degree(n)
    g = np.arange(n)
    parity = (g[:, None, None] + g[None, :, None] + g[None, None, :]) & 1
    live = den > 0.0
    d = np.zeros_like(a)
    for _ in range(sweeps):
        for colour in (0, 1):
            new = (b + lam * neighbour_sum(d)) / np.where(live, den, 1.0)
            m = (parity == colour) & live
            d[m] = new[m]
        if history is not None:
            history.append(d.copy())
    return d


def solve(sums, lam=DEFAULT_LAMBDA, sweeps=DEFAULT_SWEEPS, dtype=np.float32):
    """The LUT of hg_lut_solve: fp32 (n, n, n, 3) (dtype=np.float64: before the one rounding)."""
    n = sums.shape[0]
    lut = identity(n)
    for c in range(3):
        ab = system(sums, n, c)
        if ab is not None:
            lut[..., c] += solve_channel(ab[0], ab[1], float(lam), int(sweeps))
    return lut.astype(dtype)


def laplacian(n):
    import scipy.sparse as sp
    def path(m):
        e = np.ones(m - 1)
        deg = np.full(m, 2.0)
        deg[0] = deg[-1] = 1.0
        return sp.diags([-e, deg, -e], [-1, 0, 1])
    I, P = sp.identity(n), path(n)
    return (sp.kron(sp.kron(P, I), I) + sp.kron(sp.kron(I, P), I) + sp.kron(sp.kron(I, I), P)).tocsc()


def direct(sums, lam, dtype=np.float64):
    """The exact solution of the same system (scipy sparse LU); lam > 0."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    n = sums.shape[0]
    lut = identity(n)
    if system(sums, n, 0) is not None:
        a = system(sums, n, 0)[0]
        b = np.stack([system(sums, n, c)[1].ravel() for c in range(3)], axis=1)          # one matrix, three right-hand sides
        lut += spsolve((sp.diags(a.ravel()) + lam * laplacian(n)).tocsc(), b).reshape(n, n, n, 3)
    return lut.astype(dtype)


def residual(sums, lut, lam):
    """max over the channels of |b - (diag(a) + lam L) d| / |b| (2-norms) for d = lut - identity."""
    n = sums.shape[0]
    worst = 0.0
    for c in range(3):
        ab = system(sums, n, c)
        if ab is None or not np.any(ab[1]):
            continue
        d = np.asarray(lut, dtype=np.float64)[..., c] - identity(n)[..., c]
        r = ab[1] - (ab[0] * d + lam * (degree(n) * d - neighbour_sum(d)))
        worst = max(worst, float(np.linalg.norm(r) / np.linalg.norm(ab[1])))
    return worst


def fit(s, t, w=None, n=33, lam=DEFAULT_LAMBDA, sweeps=DEFAULT_SWEEPS, dtype=np.float32):
    return solve(splat(s, t, w, n), lam, sweeps, dtype)


# ---- .cube -------------------------------------------------------------------------------------------------------------
def cube_rows(lut):
    return np.asarray(lut, dtype=np.float32).reshape(-1, 3)


# ---- the synthetic pair ------------------------------------------------------------------------------------------------
def true_map(x):
    """g: smooth and not affine -- a per-channel gamma, a 3 x 3 mix and a hue-dependent bump.  x (..., 3) in [0, 1], fp64."""
    x = np.asarray(x, dtype=np.float64)
    y = x ** np.array([0.8, 1.1, 1.35])
    y = y @ np.array([[0.90, 0.10, 0.00], [0.05, 0.85, 0.10], [0.00, 0.15, 0.85]]).T
    u, v = x[..., 0] - x[..., 1], 0.5 * (x[..., 0] + x[..., 1]) - x[..., 2]          # opponent axes: hue = atan2(v, u)
    y[..., 0] += 0.30 * u * v                                                        # chroma^2 sin(2 hue) / 2
    y[..., 2] += 0.20 * (u * u - v * v)                                              # chroma^2 cos(2 hue)
    return y


def smooth_image(size, seed=0, blobs=5):
    """(size, size, 3) fp64 in [0, 1]: low-pass noise (a few low-frequency waves per channel) plus flat blobs."""
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, size), np.linspace(0, 1, size), indexing='ij')
    img = np.zeros((size, size, 3))
    for c in range(3):
        acc = np.zeros((size, size))
        for _ in range(6):
            fx, fy, ph, am = rs.uniform(-3, 3), rs.uniform(-3, 3), rs.uniform(0, 2 * np.pi), rs.uniform(0.3, 1.0)
            acc += am * np.sin(2 * np.pi * (fx * xx + fy * yy) + ph)
        img[..., c] = 0.5 + 0.5 * acc / np.abs(acc).max()
    for _ in range(blobs):
        cy, cx, r = rs.uniform(0.1, 0.9), rs.uniform(0.1, 0.9), rs.uniform(0.04, 0.12)
        img[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = rs.uniform(0, 1, 3)
    return img


def synthetic(seed=0, full=512, small=64):
    """(s_small, t_small, s_full, t_full) as fp32 / fp32 / fp32 / fp64: the small source is the block mean of the full one (the
    256^2 copy of a photo), the targets are g of the fp32 sources."""
    s_full = smooth_image(full, seed).astype(np.float32)
    k = full // small
    s_small = s_full.astype(np.float64).reshape(small, k, small, k, 3).mean(axis=(1, 3)).astype(np.float32)
    return s_small, true_map(s_small).astype(np.float32), s_full, true_map(s_full)


def best_affine(s, t):
    """Least-squares affine map t ~ [s 1] W on (M, 3) pixels: W (4, 3)."""
    X = np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1, 3), np.ones((s.size // 3, 1))], axis=1)
    return np.linalg.lstsq(X, np.asarray(t, dtype=np.float64).reshape(-1, 3), rcond=None)[0]


# ---- inputs of the apply tests -------------------------------------------------------------------------------------------
def random_lut(n, seed=0):
    """Non-smooth entries in [-0.5, 1.5]: an indexing slip shows."""
    return np.random.RandomState(seed).uniform(-0.5, 1.5, (n, n, n, 3)).astype(np.float32)


def apply_image(n, seed=0, H=37, W=29):
    """(H, W, 3) fp32 for a LUT of n nodes: exact 0 and 1, every node value k / (n - 1), values below 0 and above 1, NaN and
    +-inf, greys, pixels with two equal fractions (the tetrahedral ties) and pixels in the last cell of each axis."""
    rs = np.random.RandomState(seed)
    x = rs.rand(H * W, 3).astype(np.float32)
    nodes = (np.arange(n, dtype=np.float64) / (n - 1)).astype(np.float32)
    x[:n, 0], x[:n, 1], x[:n, 2] = nodes, nodes[::-1], nodes[(np.arange(n) * 7 + 3) % n]
    r = n
    special = [[0, 0, 0], [1, 1, 1], [0, 1, 0.5], [-0.25, 0.5, 1.5], [np.nan, 0.3, 0.7], [np.inf, -np.inf, 0.2],
               [0.3, np.nan, np.nan], [-1e-8, 1 + 1e-7, 0.999999]]
    x[r:r + len(special)] = np.array(special, dtype=np.float32)
    r += len(special)
    x[r:r + 40] = x[r:r + 40, :1]                                   # greys
    x[r + 40:r + 80, 1] = x[r + 40:r + 80, 0]                       # fr == fg
    x[r + 80:r + 120, 2] = x[r + 80:r + 120, 1]                     # fg == fb
    last = 1.0 - rs.rand(40, 3) / (n - 1)                           # the last cell of every axis ...
    last[np.arange(20), rs.randint(0, 3, 20)] = rs.rand(20)         # ... or of two of them
    x[r + 120:r + 160] = last.astype(np.float32)
    assert r + 160 <= H * W
    return x.reshape(H, W, 3)


def u8_image(H=24, W=32, seed=0):
    """uint8 (H, W, 3) with all 256 levels on each channel."""
    rs = np.random.RandomState(seed)
    x = rs.randint(0, 256, (H * W, 3)).astype(np.uint8)
    v = np.arange(256)
    x[:256, 0], x[:256, 1], x[:256, 2] = v, (v * 7 + 3) % 256, 255 - v
    return x.reshape(H, W, 3)


def apply_unclipped(x, lut, interpolation='tetrahedral'):
    """apply in fp64 without the final clip (for the band of the quantised comparison)."""
    n = lut.shape[0]
    big = np.asarray(lut, dtype=np.float64)
    lo, hi = min(big.min(), 0.0), max(big.max(), 1.0)
    return apply(x, (big - lo) / (hi - lo), interpolation) * (hi - lo) + lo


def quantized_check(got_u8, x, lut, interpolation, bar):
    """The rule of the quantised output: equal to (uint8)(ref * 255), except where ref * 255 lies within 255 * bar of an
    integer (before the clip, so that a value the clip pins to 0 or 1 counts only when it is that close to the boundary): there
    +-1 is allowed.  Returns (share of such values, number of values off by one inside the band); raises on anything else."""
    ref = apply(x, lut, interpolation)
    v = 255.0 * apply_unclipped(x, lut, interpolation)
    near = (np.abs(v - np.rint(v)) <= 255.0 * bar) & (v >= -255.0 * bar) & (v <= 255.0 * (1.0 + bar))
    want = quantize(ref).astype(np.int64)
    diff = np.abs(got_u8.reshape(-1, 3).astype(np.int64) - want)
    assert np.all(diff[~near] == 0), f'{int((diff[~near] != 0).sum())} quantised values differ outside the band'
    assert np.all(diff <= 1)
    return float(near.mean()), int((diff != 0).sum())
