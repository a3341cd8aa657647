"""A restatement of include/fountain_hip_vectorblur.h in numpy, and the images, motion fields and G-buffers the vector-blur tests share.

Steps 1 to 3 (half velocities, tile maxima, neighbour maxima) use float32 operations in the header's order, one numpy operation per
rounding, so their results are compared bit for bit and no decision of step 4 can flip: the tie rules, the 0.25 threshold and the rint of
the tap offsets all come from these float32 values.  Step 4's weights and sums are float64 (the tap's length d is the header's float32
square root, an input of the weights like the records)."""
import numpy as np

F32 = np.float32
TILE = 16
INF = F32(np.inf)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def params(**kw):
    p = dict(taps=16, shutter=0.5, max_radius=16.0, depth_extent=0.01)
    p.update(kw)
    return p


def workspace_bytes(w, h):
    return 16 * w * h + 2 * 16 * ((w + 15) // 16) * ((h + 15) // 16)


# ------------------------------------------------------------------ steps 1 to 3, float32
def depth_of(gb12, shape):
    if gb12 is None:
        return np.zeros(shape, F32)
    z, c = gb12[..., 9].astype(F32), gb12[..., 10].astype(F32)
    with np.errstate(invalid="ignore"):
        return np.where((c > 0) & np.isfinite(z), z, INF).astype(F32)


def velocities(motion, gb12=None, **kw):
    """dict(pixels [H, W, 4] {h.x, h.y, len, z}, tiles and neighbours [ty, tx, 4] {h.x, h.y, key, 0}), float32"""
    p = params(**kw)
    m = np.ascontiguousarray(motion, dtype=F32)
    h, w = m.shape[:2]
    s = F32(0.5) * F32(p["shutter"])
    R = F32(p["max_radius"])
    with np.errstate(all="ignore"):
        fin = np.isfinite(m[..., 0]) & np.isfinite(m[..., 1])
        hx = np.where(fin, s * m[..., 0], F32(0)).astype(F32)
        hy = np.where(fin, s * m[..., 1], F32(0)).astype(F32)
        len2 = (hx * hx).astype(F32) + (hy * hy).astype(F32)
        ln = np.sqrt(len2).astype(F32)
        over = ln > R
        k = (R / np.where(over, ln, F32(1))).astype(F32)
        hx = np.where(over, hx * k, hx).astype(F32)
        hy = np.where(over, hy * k, hy).astype(F32)
        ln = np.where(over, R, ln).astype(F32)
    pixels = np.stack([hx, hy, ln, depth_of(gb12, (h, w))], axis=-1).astype(F32)
    key = (ln * ln).astype(F32)
    ty, tx = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
    tiles = np.zeros((ty, tx, 4), F32)
    for j in range(ty):
        for i in range(tx):
            ys, xs = slice(TILE * j, min(TILE * j + TILE, h)), slice(TILE * i, min(TILE * i + TILE, w))
            kk = key[ys, xs]
            a = int(np.argmax(kk))                  # the first of the largest in the tile's row-major order = the smallest pixel index
            y, x = np.unravel_index(a, kk.shape)
            tiles[j, i] = (hx[ys, xs][y, x], hy[ys, xs][y, x], kk[y, x], 0)
    nb = np.zeros_like(tiles)
    for j in range(ty):
        for i in range(tx):
            cand = [(jj, ii) for jj in (j - 1, j, j + 1) for ii in (i - 1, i, i + 1) if 0 <= jj < ty and 0 <= ii < tx]      # ascending tile index
            best = cand[int(np.argmax([tiles[c][2] for c in cand]))]
            nb[j, i] = tiles[best]
    return dict(pixels=pixels, tiles=tiles, neighbours=nb)


def offsets(n, taps):
    """the taps' (ox, oy, d) of a tile with neighbour record n: float32 decisions"""
    out = []
    for i in range(taps):
        t = F32(2 * i + 1 - taps) / F32(taps)
        ox, oy = int(np.rint(F32(t * n[0]))), int(np.rint(F32(t * n[1])))
        out.append((ox, oy, float(np.sqrt(F32(ox * ox + oy * oy)))))
    return out


# ------------------------------------------------------------------ step 4, float64
def _cone(d, r):
    with np.errstate(all="ignore"):
        return np.where(r > d, 1.0 - d / np.where(r > d, r, 1.0), 0.0)


def _cyl(d, r):
    e0, e1 = float(F32(0.95)) * r, float(F32(1.05)) * r
    with np.errstate(all="ignore"):
        u = np.clip((d - e0) / np.where(r > 0, e1 - e0, 1.0), 0.0, 1.0)
    return np.where(r > 0, 1.0 - u * u * (3.0 - 2.0 * u), 0.0)


def _front(a, b, extent):
    with np.errstate(all="ignore"):
        soft = np.where(np.isinf(a), 0.0, np.maximum(0.0, 1.0 - (np.where(np.isinf(a), 0.0, a) - np.where(np.isinf(b), 0.0, b))
                                                     / (extent * np.maximum(np.where(np.isinf(b), 1.0, b), float(F32(1e-6))))))
    return np.where(a <= b, 1.0, soft)


def blur(rgb, motion, gb12=None, **kw):
    """-> (out float64 [H, W, 3] (a copied pixel is rgb's value), copied bool [H, W], peak float64 [H, W]: the largest |colour| among the
    pixel's centre and the taps that entered its sums, what the tests' bound scales with)"""
    p = params(**kw)
    taps, extent = int(p["taps"]), float(F32(p["depth_extent"]))
    rgb = np.ascontiguousarray(rgb, dtype=F32)
    h, w = rgb.shape[:2]
    v = velocities(motion, gb12, **kw)
    px = v["pixels"].astype(np.float64)
    c64 = rgb.astype(np.float64)
    finite = np.isfinite(rgb).all(-1)
    out = c64.copy()
    copied = np.ones((h, w), bool)
    peak = np.abs(np.where(np.isfinite(c64), c64, 0)).max(-1)
    for j in range(v["tiles"].shape[0]):
        for i in range(v["tiles"].shape[1]):
            n = v["neighbours"][j, i]
            if n[2] <= F32(0.25):
                continue
            y0, x0 = TILE * j, TILE * i
            y1, x1 = min(y0 + TILE, h), min(x0 + TILE, w)
            ys, xs = np.mgrid[y0:y1, x0:x1]
            hp, zp = px[ys, xs, 2], px[ys, xs, 3]
            wc = taps / (4.0 * np.maximum(hp, 0.5))
            W, S = wc.copy(), wc[..., None] * np.where(finite[ys, xs][..., None], c64[ys, xs], 0)
            tw = np.zeros_like(W)
            pk = peak[ys, xs].copy()
            for ox, oy, d in offsets(n, taps):
                if ox == 0 and oy == 0:
                    continue
                qy, qx = ys + oy, xs + ox
                ok = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                ok &= finite[qy, qx]
                hq, zq = px[qy, qx, 2], px[qy, qx, 3]
                wt = _front(zq, zp, extent) * _cone(d, hq) + _front(zp, zq, extent) * _cone(d, hp) + 2.0 * _cyl(d, hq) * _cyl(d, hp)
                wt = np.where(ok, wt, 0.0)
                cq = np.where(ok[..., None], c64[qy, qx], 0.0)
                W += wt
                S += wt[..., None] * cq
                tw += wt
                pk = np.maximum(pk, np.abs(cq).max(-1))
            use = finite[ys, xs] & (tw > 0)
            out[ys, xs] = np.where(use[..., None], S / W[..., None], out[ys, xs])
            copied[ys, xs] = ~use
            peak[ys, xs] = pk
    return out, copied, peak


# ------------------------------------------------------------------ what the tests share
SIZES = [(1, 7), (7, 1), (16, 16), (17, 33), (48, 48), (80, 48)]           # (w, h)
TAPS = [1, 2, 15, 16, 64]
FIELDS = ["uniform", "rotational", "fast_tile", "beyond_clamp"]


def image(w, h, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, 2.0, (h, w, 3)) ** 2).astype(F32)


def field(name, w, h, seed=2):
    """motion [H, W, 2] in pixels per frame (the half velocity at the default shutter is a quarter of it)"""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    rng = np.random.default_rng(seed)
    if name == "uniform":
        m = np.broadcast_to(np.array([22.0, -9.0]), (h, w, 2)).copy()
    elif name == "rotational":
        cx, cy = 0.5 * (w - 1), 0.5 * (h - 1)
        m = np.stack([-(ys - cy), xs - cx], axis=-1) * 1.3 + rng.uniform(-0.2, 0.2, (h, w, 2))
    elif name == "fast_tile":
        m = np.zeros((h, w, 2))
        ty, tx = (h // TILE) // 2, (w // TILE) // 2                  # a middle tile (the only one of a small image)
        m[TILE * ty:TILE * ty + TILE, TILE * tx:TILE * tx + TILE] = rng.uniform(-40.0, 40.0, m[TILE * ty:TILE * ty + TILE, TILE * tx:TILE * tx + TILE].shape)
    elif name == "beyond_clamp":
        m = rng.uniform(-200.0, 200.0, (h, w, 2))
        m[::3, ::2] = np.nan                                          # unknown motion among it
    else:
        raise KeyError(name)
    return m.astype(F32)


def gbuffer(w, h, seed=3):
    """a G-buffer of which floats 9 (depth) and 10 (coverage) matter: two depth layers split along a diagonal, a soft ramp inside the
    extent, some background"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    gb = rng.uniform(-1.0, 1.0, (h, w, 12)).astype(F32)
    z = np.where(xs + ys < (w + h) // 2, 2.0, 5.0) * (1.0 + 0.004 * rng.uniform(0, 1, (h, w)))
    gb[..., 9] = z
    gb[..., 10] = 1.0
    gb[::5, ::7, 10] = 0.0                                            # background
    gb[1::6, 2::5, 9] = np.nan
    return gb
