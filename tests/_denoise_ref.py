"""A float64 numpy restatement of the a-trous filter of include/fountain_hip_denoise.h, written from its normative text and sharing no
code with the library, with a first-order bound on the library's binary32 distance from it; a one-tap image that places a weight in
binary32's subnormal range; and the seeded synthetic inputs the denoiser tests use (test_denoise_cpu.py, test_denoise.py)."""
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
    """The filter in float64, except that every weight exp(-t) is rounded to binary32 as the header states (so weights of t beyond
    about 103.97 are 0 and those of t in (87.3, 103.97] are binary32 subnormals): rgb [H, W, 3], gb [H, W, 12] -> [H, W, 3]."""
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
                    om = np.exp(-np.where(ok, t, 0.0)).astype(np.float32).astype(np.float64)     # exp rounded once to binary32
                    wt = np.where(ok, K[jy] * K[jx] * om, 0.0)
                    num += np.where(ok[..., None], wt[..., None] * uq, 0.0)
                    den += wt
            keep = ~fin | ~(den > 0)
            u = np.where(keep[..., None], u, num / np.where(den > 0, den, 1.0)[..., None])
        return np.where(demod[..., None], u * div, u)


U = 2.0 ** -24                     # unit roundoff of binary32
TINY = 2.0 ** -149                 # the least binary32 subnormal


def reference_bound(rgb, gb, **params):
    """reference() and, per pixel and channel, a first-order bound on how far the library's binary32 evaluation of the same text may
    lie from it.  Every binary32 operation is charged a relative u = 2^-24 (and a product or weight that lands among the subnormals an
    absolute 2^-149); the error of each level's colour is carried into the next through the colour distance and the weighted sum.
    The largest terms come from the plane distance: Dp = (n . dx)^2 / (sigma_plane^2 z^2) amplifies the rounding of n . dx by
    2 sqrt(Dp) / (sigma_plane z)."""
    p = dict(DEFAULTS, **params)
    rgb = np.asarray(rgb, np.float64)
    gb = np.asarray(gb, np.float64)
    if p["levels"] == 0:
        return rgb.copy(), np.zeros(rgb.shape)
    a, n, x, z, c = gb[..., 0:3], gb[..., 3:6], gb[..., 6:9], gb[..., 9], gb[..., 10]
    cov = c > 0
    demod = bool(p["flags"] & 1) & cov
    div = np.where(a > p["albedo_eps"], a, p["albedo_eps"])
    gamma = 26 * U / (1 - 26 * U)                  # a sum of at most 25 terms, and its division
    with np.errstate(all="ignore"):
        u = np.where(demod[..., None], rgb / div, rgb)
        e = np.where(demod, U * np.abs(u).max(-1), 0.0)
        zc = np.maximum(z, 1e-6)
        kpz = 1.0 / (p["sigma_plane"] ** 2 * zc ** 2)
        for i in range(p["levels"]):
            s = 2 ** i
            kc, kn = s / p["sigma_color"] ** 2, 1.0 / p["sigma_normal"] ** 2
            m = u.sum(-1) / 3.0
            em = e + U * np.abs(u).sum(-1)
            fin = np.isfinite(u).all(-1)
            num, den = np.zeros_like(u), np.zeros(u.shape[:2])
            enum, eden = np.zeros_like(u), np.zeros(u.shape[:2])
            anum, aden = np.zeros_like(u), np.zeros(u.shape[:2])
            for jy, dy in enumerate(range(-2, 3)):
                for jx, dx in enumerate(range(-2, 3)):
                    uq, ok = _shift(u, s * dy, s * dx)
                    eq, _ = _shift(e, s * dy, s * dx)
                    nq, _ = _shift(n, s * dy, s * dx)
                    xq, _ = _shift(x, s * dy, s * dx)
                    covq, _ = _shift(cov, s * dy, s * dx)
                    mq, emq = uq.sum(-1) / 3.0, eq + U * np.abs(uq).sum(-1)
                    ok = ok & (covq == cov) & np.isfinite(uq).all(-1)
                    d = u - uq
                    ed = (e + eq)[..., None] + U * np.abs(d)
                    S = (d ** 2).sum(-1)
                    eS = (2 * np.abs(d) * ed + ed ** 2).sum(-1) + 5 * U * S
                    M = (m ** 2 + mq ** 2) / 2 + p["color_eps"]
                    eM = np.abs(m) * em + np.abs(mq) * emq + (em ** 2 + emq ** 2) / 2 + 4 * U * M
                    dc = kc * S / M
                    edc = kc * (eS + S * eM / M) / M + 6 * U * dc
                    dn = kn * ((n - nq) ** 2).sum(-1)
                    pd = (n * (x - xq)).sum(-1)
                    epd = 4 * U * (np.abs(n) * np.abs(x - xq)).sum(-1)
                    dp = pd ** 2 * kpz
                    edp = (2 * np.abs(pd) * epd + epd ** 2) * kpz + 7 * U * dp
                    t = dc + dn + dp
                    et = edc + 8 * U * dn + edp + 2 * U * t
                    ok = ok & ~np.isnan(t)
                    tt = np.where(ok, t, 0.0)
                    om = np.exp(-tt).astype(np.float32).astype(np.float64)
                    eom = np.minimum(1.0, np.exp(np.minimum(np.where(ok, et, 0.0) - tt, 0.0))) - np.exp(-tt) + 2 * U * om + TINY    # |exp(-t') - exp(-t)|, |t' - t| <= et
                    k = K[jy] * K[jx]
                    wt = np.where(ok, k * om, 0.0)
                    ewt = np.where(ok, k * eom + U * wt + TINY, 0.0)
                    num += np.where(ok[..., None], wt[..., None] * uq, 0.0)
                    den += wt
                    enum += np.where(ok[..., None], ewt[..., None] * np.abs(uq) + (wt * eq)[..., None], 0.0)
                    eden += ewt
                    anum += np.where(ok[..., None], wt[..., None] * np.abs(uq), 0.0)
                    aden += wt
            keep = ~fin | ~(den > 0)
            dd = np.where(den > 0, den, 1.0)
            un = num / dd[..., None]
            eun = (enum + gamma * anum + np.abs(un) * (eden + gamma * aden)[..., None]) / dd[..., None] + U * np.abs(un)
            u = np.where(keep[..., None], u, un)
            e = np.where(keep, e, eun.max(-1))
        out = np.where(demod[..., None], u * div, u)
        eout = np.where(demod[..., None], e[..., None] * div, e[..., None]) + U * np.abs(out)
        return out, eout


def one_tap(t_target, above=False):
    """A 1 x 5 image whose centre pixel is black and whose right neighbour is bright and coplanar, the other three pixels being
    environment (no weight): at level 0 the centre's only other tap has t = Dc + Dn, Dc about 6e-6 (sigma_color 1000) and Dn dialled
    through the neighbour's normal (sigma_normal 1).  t is the binary32 value the library computes; with above = True the first one
    beyond t_target.  Returns rgb, gb, params, t and the centre's output in the header's binary32 arithmetic:
    (3/8 * 1/4 * w) / (3/8 * 3/8), w = exp(-t) rounded to binary32 (0 when t > 104)."""
    f = np.float32
    params = dict(levels=1, flags=0, sigma_color=1000.0, sigma_normal=1.0)
    kc = f(f(1.0) / f(f(1000.0) * f(1000.0)))
    dc = f(f(kc * f(3.0)) / f(f(f(0.0) + f(1.0) * f(1.0)) * f(0.5) + f(1e-4)))

    def t_of(a):
        return f(f(dc + f(f(1.0) * f(a * a))) + f(0.0))

    a = f(np.sqrt(t_target))
    if above:
        while t_of(a) <= f(t_target):
            a = np.nextafter(a, f(np.inf))
    else:
        while t_of(a) > f(t_target):
            a = np.nextafter(a, f(0))
        while t_of(np.nextafter(a, f(np.inf))) <= f(t_target):
            a = np.nextafter(a, f(np.inf))
    t = t_of(a)
    rgb = np.zeros((1, 5, 3), f)
    rgb[0, 3] = 1.0
    rgb[0, [0, 1, 4]] = 0.5
    gb = np.zeros((1, 5, 12), f)
    gb[0, :, 5] = 1.0
    gb[0, :, 6] = np.arange(5) * 0.01
    gb[0, :, 9] = 2.0
    gb[0, :, 10:12] = 1.0
    gb[0, [0, 1, 4], 10] = 0.0
    gb[0, 3, 3] = a
    w = f(np.exp(-np.float64(t))) if t <= f(104.0) else f(0.0)
    wt = f(f(f(0.375) * f(0.25)) * w)
    want = f(f(f(0.0) + wt * f(1.0)) / f(f(f(0.375) * f(0.375)) + wt))
    return rgb, gb, params, t, want


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
