"""numpy restatement of regrain (include/hg_regrain.h; histogan_amd.post.regrain), the yardstick of tests/test_regrain_*.py.
The reference project has no regrain; the definition restates Pitie, Kokaram, Dahyot 2007 on the offset field D = J - I.

Every function takes `dtype`: np.float64 is the reference, np.float32 runs the same operations in the same order with every
one rounded to fp32 (numpy contracts nothing into a fused multiply-add), which is what the GPU tests take their error bar
from.  Internally images are planes (3, H, W).  The resize between levels is post_ref.imresize(method='bilinear'), which
computes in fp64 whatever `dtype` is; its result is rounded to `dtype`.
"""
import numpy as np

import post_ref

RHO = 0.2
MIN_SIDE = 20
ITERATIONS = (4, 16, 32, 64, 64, 64)


def levels(h, w, iterations=ITERATIONS, min_side=MIN_SIDE):
    """[(h, w), (ceil(h / 2), ceil(w / 2)), ...]: level l + 1 exists while iterations has an entry for it and both of its sides
    exceed min_side."""
    sizes = [(int(h), int(w))]
    while len(sizes) < len(iterations):
        h2, w2 = -(-sizes[-1][0] // 2), -(-sizes[-1][1] // 2)
        if not (h2 > min_side and w2 > min_side):
            break
        sizes.append((h2, w2))
    return sizes


def workspace_floats(sizes):
    """hg_regrain_workspace_bytes / 4: per level the planes I, E, a, b (3 each), coef (4), scratch (1), each rounded up to 4."""
    up = lambda n: (n + 3) // 4 * 4  # noqa: E731
    return sum(4 * up(3 * h * w) + up(4 * h * w) + up(h * w) for h, w in sizes)


def resize(planes, hw, dtype=np.float64):
    """The antialiased bilinear resize of (C, H, W) planes to hw."""
    out = post_ref.imresize(np.asarray(planes, dtype=np.float64).transpose(1, 2, 0), output_shape=hw, method='bilinear')
    return np.ascontiguousarray(out.transpose(2, 0, 1)).astype(dtype)


def gradient_magnitude(I, dtype=np.float64):
    """d (H, W) of the planes I (3, H, W): forward differences, 0 past the last column / row, summed in the header's order."""
    I = np.asarray(I, dtype=dtype)
    gx, gy = np.zeros_like(I), np.zeros_like(I)
    gx[:, :, :-1] = I[:, :, 1:] - I[:, :, :-1]
    gy[:, :-1, :] = I[:, 1:, :] - I[:, :-1, :]
    q = gx[0] * gx[0]
    q = q + gy[0] * gy[0]
    for c in (1, 2):
        q = q + gx[c] * gx[c]
        q = q + gy[c] * gy[c]
    return np.sqrt(q)


def coef(I, level, smoothness=1.0, dtype=np.float64):
    """The coefficient planes (psi, w_r, w_d, s), (4, H, W), of the level's planes I (3, H, W)."""
    t = dtype
    d = gradient_magnitude(I, t)
    psi = np.minimum(t(1), (t(256) * d) / t(5))
    phi = t(30.0 * 2.0 ** -level) / (t(1) + (t(10) * d) / t(smoothness))
    wr, wd = np.zeros_like(phi), np.zeros_like(phi)
    wr[:, :-1] = (phi[:, :-1] + phi[:, 1:]) * t(0.5)
    wd[:-1, :] = (phi[:-1, :] + phi[1:, :]) * t(0.5)
    wl, wu = np.zeros_like(phi), np.zeros_like(phi)
    wl[:, 1:] = wr[:, :-1]
    wu[1:, :] = wd[:-1, :]
    den = (((psi + wr) + wl) + wd) + wu
    s = (t(1) - t(RHO)) / den
    return np.stack([psi, wr, wd, s]).astype(t)


def sweep_once(D, E, C, dtype=np.float64):
    """One damped Jacobi sweep of D (3, h, w) with E (3, h, w) and the coefficient planes C (4, h, w).  A cell on the border of
    the arrays takes nothing from the neighbours the arrays do not hold: on a whole level that is the definition; on a window
    cropped from a level (s still divides by the full sum of weights) it is what the tiled kernel does with its staged region."""
    t = dtype
    D, E = np.asarray(D, dtype=t), np.asarray(E, dtype=t)
    psi, wr, wd, s = (np.asarray(c, dtype=t) for c in C)
    a = psi * E
    a[:, :, :-1] = a[:, :, :-1] + wr[:, :-1] * D[:, :, 1:]
    a[:, :, 1:] = a[:, :, 1:] + wr[:, :-1] * D[:, :, :-1]
    a[:, :-1, :] = a[:, :-1, :] + wd[:-1, :] * D[:, 1:, :]
    a[:, 1:, :] = a[:, 1:, :] + wd[:-1, :] * D[:, :-1, :]
    return s * a + t(RHO) * D


def sweep(D, E, C, n, dtype=np.float64):
    for _ in range(n):
        D = sweep_once(D, E, C, dtype)
    return D


def begin(original, transferred, dtype=np.float64):
    """(I, E) planes (3, H, W) of two (H, W, 3) images."""
    I = np.ascontiguousarray(np.asarray(original, dtype=dtype).transpose(2, 0, 1))
    T = np.ascontiguousarray(np.asarray(transferred, dtype=dtype).transpose(2, 0, 1))
    return I, T - I


def finish(I, D, dtype=np.float64):
    """clip(I + D, 0, 1) as (H, W, 3)."""
    return np.clip(np.asarray(I, dtype=dtype) + np.asarray(D, dtype=dtype), 0, 1).transpose(1, 2, 0)


def regrain(original, transferred, iterations=ITERATIONS, smoothness=1.0, min_side=MIN_SIDE, dtype=np.float64, clip=True):
    """regrain of two (H, W, 3) images: (H, W, 3) in `dtype`.  clip=False returns I + D_0 unclipped."""
    I, E = begin(original, transferred, dtype)
    sizes = levels(I.shape[1], I.shape[2], iterations, min_side)
    Is, Es = [I], [E]
    for hw in sizes[1:]:
        Is.append(resize(Is[-1], hw, dtype))
        Es.append(resize(Es[-1], hw, dtype))
    D = None
    for l in range(len(sizes) - 1, -1, -1):
        D = Es[l].copy() if D is None else resize(D, sizes[l], dtype)
        D = sweep(D, Es[l], coef(Is[l], l, smoothness, dtype), iterations[l], dtype)
    return finish(I, D, dtype) if clip else (I + D).transpose(1, 2, 0)


# ---- the synthetic pair of the effect test -----------------------------------------------------------------------------------
def synthetic_pair(h=96, w=128, seed=0):
    """(I, T), (h, w, 3) fp64 in [0, 1]: I = smooth ramps with a hard-edged patch; T = an affine colour map of I quantised to 24
    levels (the banding a distribution transfer leaves on ramps) plus sigma = 0.01 noise (its grain)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    u, v = xx / (w - 1.0), yy / (h - 1.0)
    I = np.stack([0.15 + 0.6 * u, 0.2 + 0.5 * v, 0.25 + 0.25 * (u + v)], -1)
    I[h // 4:h // 2, w // 3:2 * w // 3] = I[h // 4:h // 2, w // 3:2 * w // 3] * 0.4 + np.array([0.45, 0.05, 0.3])
    A = np.array([[0.8, 0.15, 0.0], [0.05, 0.7, 0.2], [0.1, 0.0, 0.85]])
    T = I @ A.T + np.array([0.05, 0.1, 0.0])
    T = np.round(T * 24) / 24 + rs.normal(0, 0.01, T.shape)
    return np.clip(I, 0, 1), np.clip(T, 0, 1)


def gradient_rms(A, B):
    """rms over both forward-difference fields of (grad A - grad B), (H, W, 3) images."""
    d = np.asarray(A, dtype=np.float64) - np.asarray(B, dtype=np.float64)
    gx, gy = d[:, 1:] - d[:, :-1], d[1:] - d[:-1]
    return float(np.sqrt((np.sum(gx * gx) + np.sum(gy * gy)) / (gx.size + gy.size)))
