"""numpy restatement of the differentiable side of include/hg_lut.h (version 118), on top of tests/lut_ref.py.

backward      the adjoint of lut_ref.apply: gx and glut in fp64; dtype=np.float32 evaluates the same formulas in fp32 arithmetic
              (its distance to the fp64 evaluation is the eps32 the GPU tests take their bars from).
int_scatter   the integer sums of hg_lut_apply_bwd exactly as the header states them: the bits of gmax, E, the rounded
              contributions, the int64 sums, the count of contributions per node and the finished fp32 glut.
smoothness    R(d) of post.lut_smoothness, its gradient by the formula of the header, and one Adam step (hg_lut_adam_step).
refine        the loop of post.lut_refine on oracle.rgbuv_hist: fp64 with truth=True, or fp32 arithmetic throughout.
"""
import numpy as np

import lut_ref as R

GRAD_BITS = 36                        # HG_LUT_GRAD_BITS
MAX_PIXELS = 1 << 26                  # hg_lut_grad_max_pixels()
BETAS, EPS = (0.9, 0.999), 1e-8       # post.LUT_ADAM_BETAS, post.LUT_ADAM_EPS


def _at(L, idx):
    return L[idx[:, 2], idx[:, 1], idx[:, 0]]


def _flat(idx, n):
    return (idx[:, 2] * n + idx[:, 1]) * n + idx[:, 0]


def _lerp(u, v, t):
    return u + t * (v - u)


def pieces(x, lut, interpolation, dtype=np.float64):
    """Per pixel of x (M, 3) fp32: the unclipped value (M, 3), the slopes s (M, 3 channels, 3 axes), the flat node indices
    (M, K) and the weights omega (M, K) in `dtype` (K = 4 or 8).  The order of a tetrahedron's axes is that of the fp32 fractions,
    as in the kernels; in fp64 the fractions themselves are the unrounded ones, and omega is what hg_lut_apply_bwd scatters."""
    n = lut.shape[0]
    L = np.asarray(lut).astype(dtype)
    i, f = R.cell(x, n, dtype)
    f32 = R.cell(x, n, np.float32)[1]
    M = len(i)
    rows = np.arange(M)
    if interpolation == 'tetrahedral':
        order = np.argsort(-f32, axis=1, kind='stable')
        idx = i.copy()
        v = [_at(L, idx)]
        nodes = [_flat(idx, n)]
        for k in range(3):
            idx[rows, order[:, k]] += 1
            v.append(_at(L, idx))
            nodes.append(_flat(idx, n))
        fs = [f[rows, order[:, k]][:, None] for k in range(3)]
        d = [v[k + 1] - v[k] for k in range(3)]
        val = ((v[0] + fs[0] * d[0]) + fs[1] * d[1]) + fs[2] * d[2]
        s = np.zeros((M, 3, 3), dtype=dtype)
        for k in range(3):
            s[rows, :, order[:, k]] = d[k]
        a, b, c = (t[:, 0] for t in fs)
        return val, s, np.stack(nodes, axis=1), np.stack([dtype(1) - a, a - b, b - c, c], axis=1)
    if interpolation != 'trilinear':
        raise ValueError(interpolation)
    corner = lambda jr, jg, jb: _at(L, i + np.array([jr, jg, jb]))
    fr, fg, fb = f[:, 0:1], f[:, 1:2], f[:, 2:3]
    V = [[[corner(jr, jg, jb) for jr in (0, 1)] for jg in (0, 1)] for jb in (0, 1)]           # V[jb][jg][jr]
    e = [[_lerp(V[jb][jg][0], V[jb][jg][1], fr) for jg in (0, 1)] for jb in (0, 1)]           # e[jb][jg]
    hh = [_lerp(e[jb][0], e[jb][1], fg) for jb in (0, 1)]
    val = _lerp(hh[0], hh[1], fb)
    dd = [[V[jb][jg][1] - V[jb][jg][0] for jg in (0, 1)] for jb in (0, 1)]
    s = np.stack([_lerp(_lerp(dd[0][0], dd[0][1], fg), _lerp(dd[1][0], dd[1][1], fg), fb),
                  _lerp(e[0][1] - e[0][0], e[1][1] - e[1][0], fb), hh[1] - hh[0]], axis=2)
    w = [np.stack([dtype(1) - f[:, c], f[:, c]], axis=1) for c in range(3)]
    nodes, omega = [], []
    for j in range(8):
        jr, jg, jb = j & 1, (j >> 1) & 1, j >> 2
        nodes.append(_flat(i + np.array([jr, jg, jb]), n))
        omega.append((w[0][:, jr] * w[1][:, jg]) * w[2][:, jb])
    return val, s, np.stack(nodes, axis=1), np.stack(omega, axis=1)


def masked_gradient(g, val):
    """gm (M, 3) fp32: g where it is finite and the unclipped value lies in [0, 1], else 0."""
    g = np.asarray(g, dtype=np.float32).reshape(-1, 3)
    with np.errstate(invalid='ignore'):
        keep = np.isfinite(g) & (val >= 0) & (val <= 1)
    return np.where(keep, g, np.float32(0)).astype(np.float32)


def input_mask(x):
    x = np.asarray(x, dtype=np.float32).reshape(-1, 3)
    with np.errstate(invalid='ignore'):
        return (x >= 0) & (x <= 1)


def backward(x, lut, g, interpolation='tetrahedral', dtype=np.float64):
    """(gx (M, 3), glut (n, n, n, 3)) in `dtype` arithmetic for x (M, 3) fp32 and g (M, 3)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 3)
    n = lut.shape[0]
    val, s, nodes, om = pieces(x, lut, interpolation, dtype)
    gm = masked_gradient(g, val).astype(dtype)
    gx = np.zeros((len(x), 3), dtype=dtype)
    for c in range(3):
        gx = gx + gm[:, c:c + 1] * s[:, c, :]
    gx = np.where(input_mask(x), dtype(n - 1) * gx, dtype(0))
    glut = np.zeros((n ** 3, 3), dtype=dtype)
    for j in range(nodes.shape[1]):
        np.add.at(glut, nodes[:, j], om[:, j:j + 1] * gm)
    return gx, glut.reshape(n, n, n, 3)


def gmax_bits(g):
    b = np.asarray(g, dtype=np.float32).reshape(-1).view(np.uint32) & np.uint32(0x7fffffff)
    b = b[b < 0x7f800000]
    return int(b.max()) if len(b) else 0


def int_scatter(x, lut, g, interpolation='tetrahedral'):
    """(bits of gmax, sums int64 (n, n, n, 3), counts int64 (n, n, n, 3), glut fp32 (n, n, n, 3), u) of hg_lut_apply_bwd."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 3)
    n = lut.shape[0]
    val, _, nodes, omega = pieces(x, lut, interpolation, np.float64)
    gm = masked_gradient(g, val)
    bits = gmax_bits(g)
    sums, counts = np.zeros((n ** 3, 3), dtype=np.int64), np.zeros((n ** 3, 3), dtype=np.int64)
    if bits == 0:
        return 0, sums.reshape(n, n, n, 3), counts.reshape(n, n, n, 3), np.zeros((n, n, n, 3), dtype=np.float32), 0.0
    E = (bits >> 23) - 126
    scaled = gm.astype(np.float64) * 2.0 ** (GRAD_BITS - E)
    for j in range(nodes.shape[1]):
        q = np.rint(omega[:, j:j + 1] * scaled).astype(np.int64)
        np.add.at(sums, nodes[:, j], q)
        np.add.at(counts, nodes[:, j], ((omega[:, j:j + 1] != 0) & (gm != 0)).astype(np.int64))
    u = 2.0 ** (E - GRAD_BITS)
    with np.errstate(over='ignore'):
        glut = (sums.astype(np.float64) * u).astype(np.float32)
    return bits, sums.reshape(n, n, n, 3), counts.reshape(n, n, n, 3), glut.reshape(n, n, n, 3), u


# ---- the smoothness term and the Adam step -----------------------------------------------------------------------------------
def identity32(n):
    """The identity as the kernels hold it: (float)((double)i / (n - 1))."""
    return R.identity(n).astype(np.float32)


def smoothness(lut, ident=None):
    """R(d) = (n - 1)^2 mean over the 3 n^2 (n - 1) edges of |d_i - d_j|^2, d = lut - identity, fp64."""
    n = lut.shape[0]
    d = np.asarray(lut, dtype=np.float64) - (R.identity(n) if ident is None else np.asarray(ident, dtype=np.float64))
    total = sum((np.diff(d, axis=ax) ** 2).sum() for ax in (0, 1, 2))
    return (n - 1) ** 2 * total / (3 * n * n * (n - 1))


def smoothness_grad(lut, dtype=np.float64, ident=None):
    """2 (n - 1)^2 / n_edges (deg_i d_i - nb_i) per node and channel, in `dtype`, d against the fp32 identity by default."""
    n = lut.shape[0]
    d = np.asarray(lut).astype(dtype) - (identity32(n) if ident is None else ident).astype(dtype)
    coef = dtype(2.0 * (n - 1) ** 2 / (3.0 * n * n * (n - 1)))
    out = np.empty_like(d)
    deg = R.degree(n).astype(dtype)
    for c in range(3):
        out[..., c] = coef * (deg * d[..., c] - R.neighbour_sum(d[..., c]))
    return out


def adam_step(lut, grad, m, v, step, lr, lam, betas=BETAS, eps=EPS, dtype=np.float64):
    """(lut, m, v) after hg_lut_adam_step, in `dtype` arithmetic; the bias corrections are fp64 host values rounded to dtype."""
    t = dtype
    lut, grad, m, v = (np.asarray(a).astype(t) for a in (lut, grad, m, v))
    n = lut.shape[0]
    total = grad
    if lam != 0:
        d = lut - identity32(n).astype(t)
        coef = t(lam * (2.0 * (n - 1) ** 2 / (3.0 * n * n * (n - 1))))
        reg = np.empty_like(d)
        deg = R.degree(n).astype(t)
        for c in range(3):
            reg[..., c] = deg * d[..., c] - R.neighbour_sum(d[..., c])
        total = grad + coef * reg
    b1, b2 = t(betas[0]), t(betas[1])
    m = b1 * m + (t(1) - b1) * total
    v = b2 * v + ((t(1) - b2) * total) * total
    step_size = t(lr / (1.0 - betas[0] ** step))
    rs = t(1.0 / np.sqrt(1.0 - betas[1] ** step))
    return lut - (step_size * m) / (np.sqrt(v) * rs + t(eps)), m, v


# ---- the refine loop -----------------------------------------------------------------------------------------------------------
def target_histogram(image, h, insz=150):
    """The fp64 oracle histogram (1, 3, h, h) of an (H, W, 3) image."""
    import torch
    from oracle.rgbuv_hist import rgbuv_hist
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(image, dtype=np.float64).transpose(2, 0, 1))[None])
    return rgbuv_hist(t, h=h, insz=insz, truth=True).numpy()


def refine(lut, image, target, h, steps, lr, lam, interpolation='tetrahedral', dtype=np.float64, insz=150):
    """(lut, losses (steps + 1,)) of post.lut_refine on the oracle histogram: image (H, W, 3) fp32 no larger than insz, target
    (1, 3, h, h).  fp64: truth=True and every LUT operation in fp64; fp32: the oracle's fp32 flow and fp32 arithmetic."""
    import torch
    from oracle.rgbuv_hist import hellinger_loss, rgbuv_hist
    H, W = image.shape[:2]
    assert max(H, W) <= insz
    x = np.asarray(image, dtype=np.float32).reshape(-1, 3)
    lut = np.asarray(lut).astype(dtype)
    m, v = np.zeros_like(lut), np.zeros_like(lut)
    tgt = torch.from_numpy(np.asarray(target).astype(dtype))
    losses = []
    for k in range(steps + 1):
        out = R.apply(x, lut, interpolation, dtype).astype(dtype)
        t = torch.from_numpy(np.ascontiguousarray(out.reshape(H, W, 3).transpose(2, 0, 1))[None]).requires_grad_(True)
        loss = hellinger_loss(tgt, rgbuv_hist(t, h=h, insz=insz, truth=dtype == np.float64))
        losses.append(float(loss.detach()))
        if k == steps:
            break
        loss.backward()
        g = t.grad.numpy()[0].transpose(1, 2, 0).reshape(-1, 3)
        _, glut = backward(x, lut, g, interpolation, dtype)
        lut, m, v = adam_step(lut, glut, m, v, k + 1, lr, lam, dtype=dtype)
    return lut, np.array(losses)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def gx_image(n, seed=0, M=4000):
    """(M, 3) fp32 pixels for the gx tests: mostly generic, plus ties, node-exact, clamped and non-finite pixels (about 3 %)."""
    rs = np.random.RandomState(seed)
    x = rs.rand(M, 3).astype(np.float32)
    nodes = (np.arange(n, dtype=np.float64) / (n - 1)).astype(np.float32)
    k = min(n, 20)
    x[:k, 0], x[:k, 1] = nodes[:k], nodes[::-1][:k]                   # node-exact on two axes
    x[20:40, 1] = x[20:40, 0]                                         # ties
    x[40:60, 2] = x[40:60, 1]
    x[60:70] = x[60:70, :1]                                           # greys
    x[70:80, 0] = -rs.rand(10).astype(np.float32)                     # clamped below
    x[80:90, 1] = 1 + rs.rand(10).astype(np.float32)                  # clamped above
    x[90], x[91], x[92] = [np.nan, 0.3, 0.7], [np.inf, 0.4, 0.2], [0.6, -np.inf, 0.1]
    x[93], x[94] = [0, 0, 0], [1, 1, 1]
    return x


def comparable(x, n, margin=1e-4):
    """Pixels where fp32 and fp64 agree about the cell and the ordering: every f and every pairwise difference of f at least
    `margin` from 0 and from 1, and every component finite and inside [0, 1]."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 3)
    _, f = R.cell(x, n)
    far = lambda t: (np.abs(t) >= margin) & (np.abs(t - 1) >= margin) & (np.abs(t + 1) >= margin)
    ok = far(f).all(1) & far(f[:, 0] - f[:, 1]) & far(f[:, 1] - f[:, 2]) & far(f[:, 0] - f[:, 2])
    return ok & input_mask(x).all(1)


def gx_comparable(x, lut, interpolation, margin=1e-4, clip=1e-5):
    """comparable(), and every unclipped output at least `clip` from 0 and 1, so that fp32 and fp64 agree on the masks too."""
    val = pieces(x, lut, interpolation)[0]
    return comparable(x, lut.shape[0], margin) & (np.minimum(np.abs(val), np.abs(val - 1)) >= clip).all(1)
