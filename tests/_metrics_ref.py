"""A float64 numpy restatement of include/fountain_hip_metrics.h, replaying the specified order: numpy's elementwise binary64 operations
are IEEE and unfused, and the pairwise tree is a reshape-and-add.  With the library's own SSIM weights (ftn_metrics_ssim_weights) every
sum is the library's bit for bit; weights() is the header's formula with Python's exp.  independent_moments() gives a second SSIM in another
summation order (scipy's 2-D correlation with the 11 x 11 outer-product kernel)."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
TILE, SUMS, TAPS, R = 16, 8, 11, 5
REC = 88                                  # bytes of a workspace record


def weights():
    e = [math.exp(-((k - 5) ** 2) / 4.5) for k in range(TAPS)]
    s = 0.0
    for v in e:
        s = s + v
    return np.array([v / s for v in e], F64)


def tiles(w, h):
    return (w + TILE - 1) // TILE, (h + TILE - 1) // TILE


def workspace_bytes(w, h):
    tx, ty = tiles(w, h)
    n = tx * ty
    total = n
    while n > 256:
        n = (n + 255) // 256
        total += n
    return 16 * ((REC * total + 15) // 16)


def pairwise(v):
    """S[0, n) over the last axis, n a power of two: adjacent pairs, level by level."""
    v = np.asarray(v, F64)
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def tile_sums(plane):
    """The tile sums [n_tiles] of a [h, w] plane whose empty slots are +0.0."""
    h, w = plane.shape
    tx, ty = tiles(w, h)
    full = np.zeros((ty * TILE, tx * TILE), F64)
    full[:h, :w] = plane
    return pairwise(full.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(ty * tx, TILE * TILE))


def total(per_tile):
    n = 1
    while n < len(per_tile):
        n *= 2
    v = np.zeros(n, F64)
    v[:len(per_tile)] = per_tile
    return float(pairwise(v))


def _sep(v, g):
    """both passes over a [h, w] plane -> [h - 10, w - 10]"""
    h, w = v.shape
    t = np.zeros((h, w - 2 * R), F64)
    for k in range(TAPS):
        t = t + g[k] * v[:, k:k + w - 2 * R]
    o = np.zeros((h - 2 * R, w - 2 * R), F64)
    for k in range(TAPS):
        o = o + g[k] * t[k:k + h - 2 * R, :]
    return o


def _ssim_of(mom, C1, C2):
    ma, mb, aa, bb, ab = mom
    va = aa - ma * ma
    vb = bb - mb * mb
    cab = ab - ma * mb
    return (((2.0 * ma) * mb + C1) * (2.0 * cab + C2)) / (((ma * ma + mb * mb) + C1) * ((va + vb) + C2))


def _constants(peak):
    k1, k2 = 0.01 * float(F32(peak)), 0.03 * float(F32(peak))
    return k1 * k1, k2 * k2


def bad_pixels(test, ref):
    return ~(np.isfinite(test).all(-1) & np.isfinite(ref).all(-1))


def windows(bad):
    """[h, w] bool: where an SSIM window exists"""
    h, w = bad.shape
    ok = np.zeros((h, w), bool)
    if h < TAPS or w < TAPS:
        return ok
    n = np.zeros((h - 2 * R, w - 2 * R), np.int64)
    for j in range(TAPS):
        for i in range(TAPS):
            n += bad[j:j + h - 2 * R, i:i + w - 2 * R]
    ok[R:h - R, R:w - R] = n == 0
    return ok


def ssim_pixels(test, ref, peak, g, moments=_sep):
    """SSIM_p [h, w] (the three channels' sum; garbage where no window exists); `moments(plane, g)` is the window's weighted sum"""
    h, w, _ = test.shape
    bad = bad_pixels(test, ref)
    C1, C2 = _constants(peak)
    out = np.zeros((h, w), F64)
    acc = None
    for c in range(3):
        a = np.where(bad, 0.0, test[..., c]).astype(F64)
        b = np.where(bad, 0.0, ref[..., c]).astype(F64)
        s = _ssim_of([moments(v, g) for v in (a, b, a * a, b * b, a * b)], C1, C2)
        acc = s if acc is None else acc + s
    out[R:h - R, R:w - R] = acc
    return out


def independent_moments(plane, g):
    from scipy import ndimage
    return ndimage.correlate(plane, np.outer(g, g), mode="constant")[R:-R, R:-R]


def reference(test, ref, peak=1.0, rel_eps=1e-2, ssim=False, g=None, moments=_sep):
    """dict(totals, result, tile_sums [n_tiles, 8], error_map, ssim_map) of the header, and ssim_pixels: SSIM_p in binary64, +0.0
    where there is no window"""
    test, ref = np.ascontiguousarray(test, F32), np.ascontiguousarray(ref, F32)
    h, w, _ = test.shape
    eps = float(F32(rel_eps))
    bad = bad_pixels(test, ref)
    good = ~bad
    with np.errstate(all="ignore"):
        a, b = test.astype(F64), ref.astype(F64)
        d = a - b
        se = d * d
        ae = np.abs(d)
        rel = se / (b * b + eps)
        sm = ae / ((np.abs(a) + np.abs(b)) + eps)
    pix = lambda v: (v[..., 0] + v[..., 1]) + v[..., 2]
    planes = [pix(se), pix(ae), pix(rel), pix(sm), se[..., 0], se[..., 1], se[..., 2]]
    planes = [np.where(good, v, 0.0) for v in planes]
    win = np.zeros((h, w), bool)
    ssim_p = np.zeros((h, w), F64)
    if ssim:
        win = windows(bad)
        with np.errstate(all="ignore"):
            ssim_p = np.where(win, ssim_pixels(test, ref, peak, weights() if g is None else g, moments), 0.0)
    planes.append(ssim_p)
    per_tile = np.stack([tile_sums(v) for v in planes], axis=1)
    sums = [total(per_tile[:, q]) for q in range(SUMS)]
    m = np.where(good, ae.max(-1), -1.0).ravel()
    at = int(np.argmax(m))                                            # the first of equals
    n_pixels, n_bad = h * w, int(bad.sum())
    tot = dict(sum=tuple(sums), max_abs=float(m[at]) if n_bad < n_pixels else 0.0, max_abs_index=at if n_bad < n_pixels else 0, n_pixels=n_pixels,
               n_nonfinite=n_bad, n_different=int((test.view(np.uint32) != ref.view(np.uint32)).any(-1).sum()), n_ssim_windows=int(win.sum()))
    with np.errstate(all="ignore"):
        err_map = np.where(good, planes[0] / 3.0, np.nan).astype(F32)
        ssim_map = np.where(win, ssim_p / 3.0, np.nan).astype(F32)
    return dict(totals=tot, result=resolve(tot, peak), tile_sums=per_tile, error_map=err_map, ssim_map=ssim_map, ssim_pixels=ssim_p)


def resolve(t, peak=1.0):
    nan = float("nan")
    n = t["n_pixels"] - t["n_nonfinite"]
    n3 = 3.0 * float(n)
    S = t["sum"]
    P = float(F32(peak))
    mean = lambda v: v / n3 if n else nan
    mse = mean(S[0])
    return dict(mse=mse, rmse=math.sqrt(mse) if n else nan, mae=mean(S[1]), rel_mse=mean(S[2]), smape=mean(S[3]),
                psnr=nan if not n else (math.inf if mse == 0.0 else 10.0 * math.log10(P * P / mse)),
                ssim=S[7] / (3.0 * float(t["n_ssim_windows"])) if t["n_ssim_windows"] else nan,
                mse_rgb=tuple(S[4 + c] / float(n) if n else nan for c in range(3)), max_abs=t["max_abs"] if n else nan,
                max_abs_index=t["max_abs_index"], n_pixels=t["n_pixels"], n=n, n_nonfinite=t["n_nonfinite"], n_different=t["n_different"],
                n_ssim_windows=t["n_ssim_windows"])


def bits64(v):
    return np.asarray(v, F64).view(np.uint64)


def bits32(v):
    return np.ascontiguousarray(v, F32).view(np.uint32)


def images(w, h, seed=1, scale=1.0, noise=0.1):
    """a random image and a noisy copy of it, [h, w, 3] float32"""
    rng = np.random.default_rng(seed * 7919 + w * 131 + h)
    ref = (scale * rng.random((h, w, 3))).astype(F32)
    test = (ref + noise * scale * rng.standard_normal((h, w, 3))).astype(F32)
    return test, ref
