"""The bloom stage of include/fountain_hip_bloom.h restated in binary64 numpy from the header's text: prefilter, down chain, up chain,
composite.  It shares no code with the library; the parameters are taken at the binary32 values the library's struct holds."""
import numpy as np

F32 = np.float32
LUM = np.array([float(F32(0.212671)), float(F32(0.715160)), float(F32(0.072169))])
KAPPA = np.array([0.125, 0.375, 0.375, 0.125])
DEFAULTS = dict(levels=6, karis=False, strength=0.04, scatter=0.7, threshold=0.0, knee=0.5, clamp_max=65504.0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    for k in ("strength", "scatter", "threshold", "knee", "clamp_max"):
        p[k] = float(F32(p[k]))
    return p


def levels_of(w, h, levels):
    n = 0
    while n < levels and (w > 1 or h > 1):
        w, h, n = (w + 1) >> 1, (h + 1) >> 1, n + 1
    return n


def workspace_bytes(w, h, levels):
    total = 0
    for _ in range(levels_of(w, h, levels)):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        total += 16 * ((12 * w * h + 15) // 16)
    return total


def luminance(v):
    return v[..., 0] * LUM[0] + v[..., 1] * LUM[1] + v[..., 2] * LUM[2]


def prefilter(img, p):
    img = np.asarray(img, np.float64)
    with np.errstate(invalid="ignore"):
        s = np.where(img > 0, np.minimum(img, p["clamp_max"]), 0.0)
    t = p["threshold"]
    if t == 0.0:
        return s
    Y, K = luminance(s), p["knee"] * t
    g = np.zeros_like(Y)
    hard = Y >= t + K
    g[hard] = Y[hard] - t
    if K > 0:
        soft = ~hard & (Y > t - K)
        g[soft] = (Y[soft] - t + K) ** 2 / (4 * K)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(g > 0, g / Y, 0.0)
    return np.where(g[..., None] > 0, s * q[..., None], 0.0)


def down(D, karis=False):
    h, w = D.shape[:2]
    ho, wo = (h + 1) >> 1, (w + 1) >> 1
    xs = np.clip(2 * np.arange(wo)[:, None] - 1 + np.arange(4), 0, w - 1)
    ys = np.clip(2 * np.arange(ho)[:, None] - 1 + np.arange(4), 0, h - 1)
    taps = D[ys[:, None, :, None], xs[None, :, None, :]]                       # [ho, wo, j, i, 3]
    wt = np.broadcast_to(KAPPA[:, None] * KAPPA[None, :], taps.shape[:-1])
    if karis:
        wt = wt / (1.0 + luminance(taps))
        return (wt[..., None] * taps).sum(axis=(2, 3)) / wt.sum(axis=(2, 3))[..., None]
    return (wt[..., None] * taps).sum(axis=(2, 3))


def up(C, w, h):
    hc, wc = C.shape[:2]

    def axis(n, nc):
        x = np.arange(n)
        x0 = (x - 1) >> 1
        idx = np.stack([np.clip(x0, 0, nc - 1), np.clip(x0 + 1, 0, nc - 1)], axis=-1)
        f = np.where((x & 1)[:, None] == 1, np.array([0.75, 0.25]), np.array([0.25, 0.75]))
        return idx, f
    ix, fx = axis(w, wc)
    iy, fy = axis(h, hc)
    taps = C[iy[:, None, :, None], ix[None, :, None, :]]                       # [h, w, j, i, 3]
    wt = fy[:, None, :, None] * fx[None, :, None, :]
    return (wt[..., None] * taps).sum(axis=(2, 3))


def pyramid(img, p):
    """P, B and L of the header's steps 1 to 3 (B is None when L == 0)"""
    h, w = img.shape[:2]
    P = prefilter(img, p)
    L = levels_of(w, h, p["levels"])
    if L == 0:
        return P, None, 0
    D = [P]
    for k in range(L):
        D.append(down(D[k], karis=p["karis"] and k == 0))
    U = D[L]
    for k in range(L - 1, 0, -1):
        U = D[k] * (1.0 - p["scatter"]) + up(U, D[k].shape[1], D[k].shape[0]) * p["scatter"]
    return P, up(U, w, h), L


def bloom(img, p):
    """out of step 4, binary64; channels that are not finite or are below 0 stay what they were"""
    img64 = np.asarray(img, np.float64)
    P, B, L = pyramid(img, p)
    if L == 0 or p["strength"] == 0.0:
        return img64.copy()
    with np.errstate(invalid="ignore"):
        keep = ~np.isfinite(img64) | (img64 < 0)
        return np.where(keep, img64, img64 + p["strength"] * (B - P))
