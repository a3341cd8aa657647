"""A float64 numpy restatement of the a-trous filter of include/fountain_hip_denoise.h, written from its normative text and sharing no
code with the library, and the seeded synthetic inputs the denoiser tests use (test_denoise_cpu.py, test_denoise.py)."""
import numpy as np

K = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
DEFAULTS = dict(levels=5, flags=1, sigma_color=2.0, sigma_normal=0.3, sigma_plane=1e-4, albedo_eps=1e-3, color_eps=1e-4)


def _shift(a, dy, dx):
    """a[y + dy, x + dx] where that is inside the image (zero elsewhere), and the mask of where it is"""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    ok = np.zeros((h, w), bool)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if abs(dy) < h and abs(dx) < w:
        out[yd, xd] = a[ys, xs]
        ok[yd, xd] = True
    return out, ok


def reference(rgb, gb, **params):
    """The filter in float64: rgb [H, W, 3], gb [H, W, 12] -> [H, W, 3]."""
    p = dict(DEFAULTS, **params)
    rgb = np.asarray(rgb, np.float64)
    gb = np.asarray(gb, np.float64)
    if p["levels"] == 0:
        return rgb.copy()
    a, n, x, z, c = gb[..., 0:3], gb[..., 3:6], gb[..., 6:9], gb[..., 9], gb[..., 10]
    cov = c > 0
    demod = bool(p["flags"] & 1) & cov
    div = np.where(a > p["albedo_eps"], a, p["albedo_eps"])
    with np.errstate(all="ignore"):
        u = np.where(demod[..., None], rgb / div, rgb)
        zc = np.maximum(z, 1e-6)
        for i in range(p["levels"]):
            s = 2 ** i
            m = u.sum(-1) / 3.0
            fin = np.isfinite(u).all(-1)
            num = np.zeros_like(u)
            den = np.zeros(u.shape[:2])
            for jy, dy in enumerate(range(-2, 3)):
                for jx, dx in enumerate(range(-2, 3)):
                    uq, ok = _shift(u, s * dy, s * dx)
                    nq, _ = _shift(n, s * dy, s * dx)
                    xq, _ = _shift(x, s * dy, s * dx)
                    covq, _ = _shift(cov, s * dy, s * dx)
                    mq = uq.sum(-1) / 3.0
                    ok = ok & (covq == cov) & np.isfinite(uq).all(-1)
                    dc = s * ((u - uq) ** 2).sum(-1) / (p["sigma_color"] ** 2 * ((m ** 2 + mq ** 2) / 2 + p["color_eps"]))
                    dn = ((n - nq) ** 2).sum(-1) / p["sigma_normal"] ** 2
                    dp = (n * (x - xq)).sum(-1) ** 2 / (p["sigma_plane"] ** 2 * zc ** 2)
                    t = dc + dn + dp
                    ok = ok & ~np.isnan(t)
                    wt = np.where(ok, K[jy] * K[jx] * np.exp(-np.where(ok, t, 0.0)), 0.0)
                    num += np.where(ok[..., None], wt[..., None] * uq, 0.0)
                    den += wt
            keep = ~fin | ~(den > 0)
            u = np.where(keep[..., None], u, num / np.where(den > 0, den, 1.0)[..., None])
        return np.where(demod[..., None], u * div, u)


# ------------------------------------------------------------------ synthetic inputs
def gbuffer(h, w, rng, kind="mixed"):
    """Resolved G-buffer [h, w, 12] with step edges.  kind: 'flat' (one plane, constant albedo), 'normal' (n (0,0,1) left of the middle,
    (1,0,0) right), 'coverage' (right half is environment), 'planes' (parallel planes, the right one nearer by half the depth),
    'albedo' (one plane, albedo 0.8 left / 0.2 right), 'mixed' (all of these edges in one image)."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    g = np.zeros((h, w, 12))
    g[..., 0:3] = 0.6
    g[..., 5] = 1.0
    g[..., 6], g[..., 7] = xx * 0.01, yy * 0.01
    g[..., 9] = 2.0
    g[..., 10] = 1.0
    g[..., 11] = 1.0
    right = xx >= w // 2
    if kind in ("normal", "mixed"):
        sel = right if kind == "normal" else (right & (yy < h // 2))
        g[sel, 3:6] = (1.0, 0.0, 0.0)
        g[sel, 6], g[sel, 7], g[sel, 8] = 0.5, yy[sel] * 0.01, xx[sel] * 0.01
    if kind in ("planes", "mixed"):
        sel = right if kind == "planes" else (~right & (yy >= h // 2))
        g[sel, 8] = 1.0
        g[sel, 9] = 1.0
    if kind in ("albedo", "mixed"):
        sel = right if kind == "albedo" else (xx < w // 4)
        g[sel, 0:3] = (0.8, 0.7, 0.6) if kind == "albedo" else (0.15, 0.3, 0.9)
        if kind == "albedo":
            g[~right, 0:3] = 0.2
    if kind in ("coverage", "mixed"):
        sel = right if kind == "coverage" else (right & (yy >= h // 2) & (xx >= (3 * w) // 4))
        g[sel, 0:10] = 0.0
        g[sel, 9] = np.inf
        g[sel, 10] = 0.0
    return g.astype(np.float32)


def truth(gb, rng_or_none=None):
    """Noise-free beauty: albedo times a per-region irradiance (environment pixels carry a constant sky colour)."""
    g = gb.astype(np.float64)
    irr = 0.5 + 0.3 * g[..., 5:6] - 0.2 * (g[..., 9:10] < 1.5)
    out = g[..., 0:3] * irr
    sky = g[..., 10] == 0
    out[sky] = (0.3, 0.45, 0.7)
    return out.astype(np.float32)


def gamma_noise(clean, rng, samples=4, shape=0.25):
    """The mean of `samples` gamma(shape) draws per channel, each with mean `clean` (about what 4 spp of path tracing looks like)."""
    c = np.asarray(clean, np.float64)
    d = rng.gamma(shape, 1.0 / shape, size=(samples,) + c.shape).mean(axis=0)
    return (c * d).astype(np.float32)


def synthetic(h, w, seed, kind="mixed"):
    rng = np.random.default_rng(seed)
    gb = gbuffer(h, w, rng, kind)
    clean = truth(gb)
    return gamma_noise(clean, rng), gb, clean
