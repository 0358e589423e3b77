"""The iterative distribution transfer of include/hg_post.h (hg_idt_*) restated in numpy: the definition the HIP kernels are
held to.  Every floating-point step takes a `dtype`, so the same code runs in fp64 (the reference) and in fp32 arithmetic (the
operator's own noise floor at the kernels' precision); the integer parts -- histograms, prefix sums, the quantile search --
are Python integers either way and exact.  Also here: the sliced Wasserstein-1 distance the behaviour tests measure with,
and the seeded image pairs."""
import bisect

import numpy as np

UNITS = 65536
DEGENERATE = 2.0 ** -20


def rotations(iterations, seed=0):
    """post.idt_rotations, restated: identity, then sign-fixed QR factors of normal matrices, made proper."""
    rs = np.random.RandomState(seed)
    out = [np.eye(3)]
    for _ in range(1, iterations):
        q, r = np.linalg.qr(rs.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out.append(q)
    return np.stack(out)


def project(x, R, dtype=np.float64):
    """(N, 3) projections v[:, a] = R[a] . x of (N, 3) pixels, in `dtype` (the rotation rounded to fp32 first: it is what the
    kernels are given)."""
    x = np.asarray(x).astype(dtype)
    R = np.asarray(R).astype(np.float32).astype(dtype)
    return np.stack([(R[a, 0] * x[:, 0] + R[a, 1] * x[:, 1]) + R[a, 2] * x[:, 2] for a in range(3)], axis=1)


def ranges(v):
    """(lo (3,), hi (3,)) of projections (N, 3)."""
    return v.min(axis=0), v.max(axis=0)


def nodes(v, lo, hi, n, dtype=np.float64):
    """Step 2's (k, t) of one axis' projections; every pixel of a degenerate axis sits on node 0."""
    v, lo, hi = np.asarray(v).astype(dtype), dtype(lo), dtype(hi)
    if not (hi - lo > dtype(DEGENERATE)):
        return np.zeros(v.shape, dtype=np.int64), np.zeros(v.shape, dtype=dtype)
    u = (v - lo) * dtype(n - 1) / (hi - lo)
    u = np.clip(u, dtype(0), dtype(n - 1))
    k = np.minimum(np.floor(u).astype(np.int64), n - 2)
    return k, (u - k.astype(dtype)).astype(dtype)


def histogram(v, lo, hi, n, dtype=np.float64):
    """The linear-binned fixed-point histogram of one axis: int64 (n,), summing to 65536 N exactly."""
    k, t = nodes(v, lo, hi, n, dtype)
    q = np.floor(t * dtype(UNITS) + dtype(0.5)).astype(np.int64)
    h = np.zeros(n, dtype=np.int64)
    np.add.at(h, k, UNITS - q)
    np.add.at(h, k + 1, q)
    return h


def quantile_map(h0, h1, lo1, hi1):
    """Step 3: M (n,) in fp64 (the kernels store it as fp32) from two integer histograms and the target's range."""
    h0, h1 = [int(c) for c in h0], [int(c) for c in h1]
    n = len(h0)
    c0, c1 = list(np.cumsum(np.array(h0, dtype=object))), list(np.cumsum(np.array(h1, dtype=object)))
    T0, T1 = c0[-1], c1[-1]
    rhs = [c * T0 for c in c1]
    lo1, hi1 = float(lo1), float(hi1)
    M = np.empty(n, dtype=np.float64)
    for k in range(n):
        lhs = c0[k] * T1
        j = min(bisect.bisect_left(rhs, lhs), n - 1)
        up = 0.0
        if j > 0:
            den = rhs[j] - rhs[j - 1]
            up = float(j - 1) + (float(lhs - rhs[j - 1]) / float(den) if den > 0 and lhs >= rhs[j - 1] else 0.0)
        M[k] = lo1 + up / float(n - 1) * (hi1 - lo1)
    return M


def apply_maps(x, R, lo0, hi0, M, n, rho=1.0, dtype=np.float64):
    """Steps 4, 5 and the update: (N, 3) pixels moved by rho R^T d.  M: (3, n) maps, taken into `dtype`."""
    x = np.asarray(x).astype(dtype)
    Rd = np.asarray(R).astype(np.float32).astype(dtype)
    v = project(x, R, dtype)
    d = np.zeros_like(v)
    for a in range(3):
        if not (dtype(hi0[a]) - dtype(lo0[a]) > dtype(DEGENERATE)):
            continue
        k, t = nodes(v[:, a], lo0[a], hi0[a], n, dtype)
        Ma = np.asarray(M[a]).astype(dtype)
        d[:, a] = ((dtype(1) - t) * Ma[k] + t * Ma[k + 1]) - v[:, a]
    upd = np.stack([(Rd[0, c] * d[:, 0] + Rd[1, c] * d[:, 1]) + Rd[2, c] * d[:, 2] for c in range(3)], axis=1)
    return (x + dtype(rho) * upd).astype(dtype)


def target_tables(tgt, rots, n, dtype=np.float64):
    """Per rotation (lo1, hi1, [h1 of the three axes]) of the target pixels (N1, 3)."""
    out = []
    for R in rots:
        w = project(tgt, R, dtype)
        lo1, hi1 = ranges(w)
        out.append((lo1, hi1, [histogram(w[:, a], lo1[a], hi1[a], n, dtype) for a in range(3)]))
    return out


def transfer(source, target, rots, bins, rho=1.0, dtype=np.float64, clip=True):
    """The whole operator on (H, W, 3) or (N, 3) arrays: the source pixels after every rotation, clipped to [0, 1]."""
    shape = np.asarray(source).shape
    x = np.asarray(source).astype(np.float32).astype(dtype).reshape(-1, 3)
    y = np.asarray(target).astype(np.float32).astype(dtype).reshape(-1, 3)
    tabs = target_tables(y, rots, bins, dtype)
    for R, (lo1, hi1, h1) in zip(rots, tabs):
        v = project(x, R, dtype)
        lo0, hi0 = ranges(v)
        M = np.stack([quantile_map(histogram(v[:, a], lo0[a], hi0[a], bins, dtype), h1[a], lo1[a], hi1[a])
                      for a in range(3)]).astype(dtype)       # fp32 arithmetic stores the map as fp32, as the kernels do
        x = apply_maps(x, R, lo0, hi0, M, bins, rho, dtype)
    if clip:
        x = np.clip(x, dtype(0), dtype(1))
    return x.reshape(shape)


def _w1(a, b):
    """Wasserstein-1 distance of two 1-D samples of any two sizes: the integral of |F_a - F_b|."""
    a, b = np.sort(a), np.sort(b)
    allv = np.sort(np.concatenate([a, b]))
    dx = np.diff(allv)
    fa = np.searchsorted(a, allv[:-1], side='right') / a.size
    fb = np.searchsorted(b, allv[:-1], side='right') / b.size
    return float(np.sum(np.abs(fa - fb) * dx))


def sliced_w1(a, b, rots):
    """Mean Wasserstein-1 distance of the 1-D marginals of two pixel sets along every axis of every rotation, fp64."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3)
    tot = 0.0
    for R in rots:
        pa, pb = a @ np.asarray(R, dtype=np.float64).T, b @ np.asarray(R, dtype=np.float64).T
        tot += sum(_w1(pa[:, c], pb[:, c]) for c in range(3))
    return tot / (3 * len(rots))


HELD_OUT_SEED = 1234       # rotations the transfer never saw: what sliced_w1 is measured along
SRC_HW, TGT_HW = (32, 40), (32, 32)        # 1280 and 1024 pixels: bins <= 64 keeps bins <= pixels / 16 for both


def held_out(k=8):
    return rotations(k + 1, HELD_OUT_SEED)[1:]


def seeded_pair(kind, seed=0):
    """(source (32, 40, 3), target (32, 32, 3)) fp32 images in [0, 1]: a smooth textured source, and a target whose colour
    distribution is 'smooth' (one correlated blob) or 'bimodal' (two separated clusters: what an affine map cannot reach)."""
    rs = np.random.RandomState(100 + seed)
    H, W = SRC_HW
    yy, xx = np.mgrid[0:H, 0:W] / float(max(H, W))
    src = np.stack([0.5 + 0.25 * np.sin(5 * yy + 1) * np.cos(4 * xx), 0.45 + 0.3 * yy * xx + 0.1 * np.cos(7 * xx),
                    0.4 + 0.2 * np.cos(3 * yy - 2 * xx)], axis=-1) + rs.normal(0, 0.05, (H, W, 3))
    h, w = TGT_HW
    # bounded supports, and a bridge between the two modes: no projection of the target leaves histogram nodes empty at
    # 64 bins, where the quantile map would be discontinuous in the counts ("Conditioning")
    A = np.array([[0.30, 0.08, 0.03], [0.0, 0.22, 0.06], [0.0, 0.0, 0.16]])
    if kind == 'smooth':
        tgt = 0.5 + rs.uniform(-1, 1, (h * w, 3)) @ A
    elif kind == 'bimodal':
        c0, c1 = np.array([0.27, 0.58, 0.68]), np.array([0.75, 0.36, 0.26])
        u = rs.rand(h * w)
        s = np.where(u < 0.42, 0.0, np.where(u < 0.84, 1.0, rs.rand(h * w)))          # 42 % / 42 % modes, 16 % bridge
        tgt = c0 + s[:, None] * (c1 - c0) + rs.uniform(-1, 1, (h * w, 3)) @ (0.45 * A)
    else:
        raise ValueError(kind)
    return np.clip(src, 0, 1).astype(np.float32), np.clip(tgt.reshape(h, w, 3), 0, 1).astype(np.float32)
