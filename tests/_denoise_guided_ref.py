"""A float64 numpy restatement of the variance-guided a-trous filter of include/fountain_hip_denoise_guided.h, written from its normative
text and sharing no code with the library, and a seeded synthetic generator that draws explicit per-pixel samples, so that var4 is the
true unbiased variance of each pixel's mean (test_denoise_guided_cpu.py, test_denoise_guided.py)."""
import numpy as np

import _denoise_ref as DR

K = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
K3 = np.array([0.25, 0.5, 0.25])
DEFAULTS = dict(levels=5, flags=1, sigma_variance=2.0, sigma_normal=0.3, sigma_plane=0.1, albedo_eps=1e-3, rel_eps=1e-4)

_shift = DR._shift


def reference(rgb, gb, var4, geometry_only=False, **params):
    """The filter in float64, except that every weight exp(-t) is rounded to binary32 as the header states (weights of t beyond about
    103.97 are 0): rgb [H, W, 3], gb [H, W, 12], var4 [H, W, 4] -> [H, W, 3].  With geometry_only every colour term is 0 (the filter
    the header defines for var4 = +inf everywhere)."""
    p = dict(DEFAULTS, **params)
    rgb = np.asarray(rgb, np.float64)
    gb = np.asarray(gb, np.float64)
    var = np.asarray(var4, np.float64)[..., 0:3]
    if p["levels"] == 0:
        return rgb.copy()
    a, n, x, z, c = gb[..., 0:3], gb[..., 3:6], gb[..., 6:9], gb[..., 9], gb[..., 10]
    cov = c > 0
    demod = bool(p["flags"] & 1) & cov
    div = np.where(a > p["albedo_eps"], a, p["albedo_eps"])
    d = np.where(demod[..., None], div, 1.0)
    kv = 2.0 * p["sigma_variance"] ** 2
    with np.errstate(all="ignore"):
        u = rgb / d
        nu = (var / d ** 2).sum(-1)
        nu = np.where((var >= 0).all(-1), nu, np.nan)                 # NaN or negative variances: the pixel is not usable
        zc = np.maximum(z, 1e-6)
        for i in range(p["levels"]):
            s = 2 ** i
            usable = np.isfinite(u).all(-1) & ~np.isnan(nu)
            # a. the 3 x 3 prefilter of nu at unit offsets
            sv, sk = np.zeros(nu.shape), np.zeros(nu.shape)
            for jy, dy in enumerate(range(-1, 2)):
                for jx, dx in enumerate(range(-1, 2)):
                    nq, ok = _shift(nu, dy, dx)
                    uoq, _ = _shift(usable, dy, dx)
                    covq, _ = _shift(cov, dy, dx)
                    ok = ok & uoq & (covq == cov)
                    k = K3[jy] * K3[jx]
                    sv += np.where(ok, k * np.where(ok, nq, 0.0), 0.0)
                    sk += np.where(ok, k, 0.0)
            nuh = sv / np.where(sk > 0, sk, 1.0)
            m = u.sum(-1) / 3.0
            den = kv * nuh + p["rel_eps"] * m ** 2
            # b. the 25 taps
            num, wsum, snu = np.zeros_like(u), np.zeros(nu.shape), np.zeros(nu.shape)
            for jy, dy in enumerate(range(-2, 3)):
                for jx, dx in enumerate(range(-2, 3)):
                    uq, ok = _shift(u, s * dy, s * dx)
                    nuq, _ = _shift(nu, s * dy, s * dx)
                    uoq, _ = _shift(usable, s * dy, s * dx)
                    nq, _ = _shift(n, s * dy, s * dx)
                    xq, _ = _shift(x, s * dy, s * dx)
                    covq, _ = _shift(cov, s * dy, s * dx)
                    ok = ok & (covq == cov) & uoq
                    d2 = ((u - uq) ** 2).sum(-1)
                    if geometry_only:
                        dc = np.zeros(d2.shape)
                    else:
                        dc = np.where((d2 == 0) | np.isinf(nuh), 0.0, d2 / den)       # d2 / 0 = +inf (weight 0)
                    dn = ((n - nq) ** 2).sum(-1) / p["sigma_normal"] ** 2
                    dp = (n * (x - xq)).sum(-1) ** 2 / (p["sigma_plane"] ** 2 * zc ** 2)
                    t = dc + dn + dp
                    ok = ok & ~np.isnan(t)
                    om = np.exp(-np.where(ok, t, 0.0)).astype(np.float32).astype(np.float64)     # exp rounded once to binary32
                    wt = np.where(ok, K[jy] * K[jx] * om, 0.0)
                    ok = ok & (wt > 0)
                    num += np.where(ok[..., None], wt[..., None] * uq, 0.0)
                    wsum += np.where(ok, wt, 0.0)
                    snu += np.where(ok, wt * wt * np.where(ok, nuq, 0.0), 0.0)
            keep = ~usable | ~(wsum > 0)
            ws = np.where(wsum > 0, wsum, 1.0)
            u = np.where(keep[..., None], u, num / ws[..., None])
            nu = np.where(keep, nu, snu / ws ** 2)
        return u * d


# ------------------------------------------------------------------ synthetic inputs with explicit samples
def sample_gamma(clean, rng, samples, shape=0.25):
    """`samples` gamma(shape) draws per pixel and channel, each with mean `clean`: [samples, H, W, 3] float64"""
    c = np.asarray(clean, np.float64)
    return c * rng.gamma(shape, 1.0 / shape, size=(samples,) + c.shape)


def mean_and_var4(s):
    """the float32 mean of the samples and var4 (r, g, b, Y = the mean of r, g, b): the unbiased variance of the mean, +inf below 2
    samples"""
    n = s.shape[0]
    mean = s.mean(0)
    y = s.mean(-1)
    if n < 2:
        var = np.full(s.shape[1:3] + (4,), np.inf)
    else:
        var = np.concatenate([s.var(0, ddof=1), y.var(0, ddof=1)[..., None]], -1) / n
    return mean.astype(np.float32), var.astype(np.float32)


def synthetic(h, w, seed, kind="mixed", samples=4, amplitude=None):
    """(rgb, gb, var4, clean): the G-buffer and noise-free truth of _denoise_ref, `samples` gamma(0.25) samples per pixel with mean
    `clean` and their mean and var4.  `amplitude` ([H, W] or None) scales each pixel's noise about its clean value (and its variance by
    the square)."""
    rng = np.random.default_rng(seed)
    gb = DR.gbuffer(h, w, rng, kind)
    clean = DR.truth(gb).astype(np.float64)
    s = sample_gamma(clean, rng, samples)
    if amplitude is not None:
        s = clean + np.asarray(amplitude, np.float64)[..., None] * (s - clean)
    rgb, var4 = mean_and_var4(s)
    return rgb, gb, var4, clean.astype(np.float32)
