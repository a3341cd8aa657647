"""A float64 numpy restatement of include/fountain_hip_temporal.h that shares no code with the library, and synthetic frames to run it on:
analytic pinhole cameras over one plane or over two planes at different depths, G-buffers and per-pixel samples generated from them so
that var4 is the variance of the pixel's mean as ftn_moments_resolve would estimate it.

The restatement also marks the pixels where a binary32 rounding may flip a discrete outcome (`fragile`): a tolerance test within 1e-4
relative of its threshold, a sample position within 1e-4 of an integer or of the image's border, a total tap weight below 0.02, a point
within 1e-4 of the previous camera's plane.  Comparisons leave those out and count them.
"""
import ctypes as C

import numpy as np

DEMODULATE = 1
# An error of about 1e-5 pixel in a binary32 sample position (raster coordinates of a few hundred, a handful of roundings) moves the
# normalised tap weights b / W by 1e-5 / W: where the taps that count weigh less than this together, history exists or not by a hair and
# its value is ill-conditioned.
W_FRAGILE = 0.02
DEFAULTS = dict(flags=DEMODULATE, alpha_min=0.4, normal_tol=0.01, plane_tol=1e-3, albedo_eps=1e-3, albedo_tol=0.01)


# ------------------------------------------------------------------ cameras
def pinhole(eye, res, focal, yaw=0.0, pitch=0.0, near=0.01):
    """A pinhole camera at `eye` looking down +z, turned by yaw (about y) and pitch (about x), radians; focal length in pixels, principal
    point at the image centre.  The four matrices are rounded to binary32, as the library will see them, and kept as float64."""
    w, h = res
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    rot = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    c2w = np.eye(4)
    c2w[:3, :3] = rot
    c2w[:3, 3] = eye
    c2r = np.array([[focal, 0, w / 2.0, 0], [0, focal, h / 2.0, 0], [0, 0, 1, -near], [0, 0, 1, 0]], dtype=np.float64)
    r32 = lambda m: m.astype(np.float32).astype(np.float64)
    return dict(c2w=r32(c2w), w2c=r32(np.linalg.inv(c2w)), r2c=r32(np.linalg.inv(c2r)), c2r=r32(c2r), eye=np.asarray(eye, np.float64),
                focal=float(focal), res=(w, h))


def camera_desc(A, cam):
    """the ftn_camera_desc of a pinhole() camera (matrices column-major, as ftn_transform keeps them)"""
    d = A.ftn_camera_desc()
    flat = lambda m: (C.c_float * 16)(*[float(v) for v in m.T.reshape(-1)])
    d.camera_to_world.m, d.camera_to_world.inv = flat(cam["c2w"]), flat(cam["w2c"])
    d.raster_to_camera.m, d.raster_to_camera.inv = flat(cam["r2c"]), flat(cam["c2r"])
    d.shutter_open, d.shutter_close, d.lens_radius, d.focal_dist = 0.0, 1.0, 0.0, 1e6
    return d


def film_desc(A, res, origin=(0, 0), full=None):
    """an ftn_film_desc whose crop is res = (w, h) at `origin`"""
    d = A.ftn_film_desc()
    w, h = res
    x0, y0 = origin
    full = full or (x0 + w, y0 + h)
    d.full_resolution = (C.c_int32 * 2)(*full)
    d.crop = (C.c_int32 * 4)(x0, y0, x0 + w, y0 + h)
    d.filter_radius = (C.c_float * 2)(0.5, 0.5)
    return d


def _apply(m, v, w1):
    """m (4 x 4) applied to v [..., 3] extended by w1; returns the homogeneous [..., 4]"""
    return v @ m[:, :3].T + w1 * m[:, 3]


def _point(m, v):
    hom = _apply(m, v, 1.0)
    with np.errstate(all="ignore"):
        return hom[..., :3] / hom[..., 3:4]


def _vector(m, v):
    return _apply(m, v, 0.0)[..., :3]


def project(cam, v, is_point):
    """world-space points (is_point) or directions -> raster x, y and camera-space depth"""
    q = np.where(is_point[..., None], _point(cam["w2c"], v), _vector(cam["w2c"], v))
    r = _point(cam["c2r"], q)
    return r[..., 0], r[..., 1], q[..., 2]


def pixel_directions(cam, h, w, origin=(0, 0), jitter=None):
    """world-space directions through the pixel centres (plus `jitter` [h, w, 2] pixels)"""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    px, py = xs + origin[0] + 0.5, ys + origin[1] + 0.5
    if jitter is not None:
        px, py = px + jitter[..., 0], py + jitter[..., 1]
    return _vector(cam["c2w"], _point(cam["r2c"], np.stack([px, py, np.zeros_like(px)], -1)))


# ------------------------------------------------------------------ synthetic frames
def texture(X, k=1.5):
    """a smooth colour of world position, in 0.2 .. 1.0 per channel; its second derivatives are at most 0.4 k^2 in size"""
    return np.stack([0.6 + 0.4 * np.sin(k * X[..., 0] + 0.3) * np.cos(k * X[..., 1]),
                     0.6 + 0.4 * np.cos(k * X[..., 0]) * np.sin(k * X[..., 1] + 0.7),
                     0.6 + 0.4 * np.sin(k * (X[..., 0] + X[..., 1]))], -1)


def albedo_of(X):
    return np.stack([0.5 + 0.3 * np.sin(0.7 * X[..., 0]), 0.5 + 0.3 * np.cos(0.9 * X[..., 1]), 0.4 + 0.2 * np.sin(0.5 * (X[..., 0] - X[..., 1]))], -1)


LUMA = np.array([0.212671, 0.715160, 0.072169])


def make_frame(cam, planes, h, w, origin=(0, 0), spp=4, sigma=0.2, seed=0, jitter=0.3, normal_noise=0.0, colour=None):
    """One frame of planes z = plane["z"] (visible where plane["xmin"] <= x <= plane["xmax"], the nearest wins; pixels that see none are
    uncovered).  The G-buffer position is where a ray `jitter` pixels off the centre hits; radiance samples are the plane's colour
    (`colour`(X), or plane["colour"], or texture(X)) times albedo noise of relative size sigma; rgb is their mean and var4 the unbiased
    sample variance over spp (+inf for spp = 1).  Returns (rgb, gb12, var4) as float32."""
    rng = np.random.default_rng(seed)
    jit = rng.uniform(-jitter, jitter, (h, w, 2)) if jitter else None
    D = pixel_directions(cam, h, w, origin, jit)
    eye = cam["eye"]
    best_t = np.full((h, w), np.inf)
    which = np.full((h, w), -1)
    for i, pl in enumerate(planes):
        with np.errstate(all="ignore"):
            t = (pl["z"] - eye[2]) / D[..., 2]
        X = eye + t[..., None] * D
        ok = (t > 0) & (t < best_t) & (X[..., 0] >= pl.get("xmin", -np.inf)) & (X[..., 0] <= pl.get("xmax", np.inf))
        best_t = np.where(ok, t, best_t)
        which = np.where(ok, i, which)
    cov = which >= 0
    X = np.where(cov[..., None], eye + np.where(cov, best_t, 0.0)[..., None] * D, 0.0)
    gb = np.zeros((h, w, 12))
    alb = albedo_of(X)
    nrm = np.zeros((h, w, 3))
    nrm[..., 2] = -1.0
    if normal_noise:
        nrm[..., :2] = rng.uniform(-normal_noise, normal_noise, (h, w, 2))
        nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    depth = _point(cam["w2c"], X)[..., 2]
    gb[..., 0:3], gb[..., 3:6], gb[..., 6:9], gb[..., 9], gb[..., 10] = alb, nrm, X, depth, 1.0
    gb[~cov] = 0.0
    gb[..., 11] = spp
    base = np.zeros((h, w, 3))
    for i, pl in enumerate(planes):
        c = colour(X) if colour is not None else (np.broadcast_to(np.asarray(pl["colour"], np.float64), X.shape) if "colour" in pl else texture(X))
        base = np.where((which == i)[..., None], c, base)
    base = np.where(cov[..., None], base, 0.3)                                   # a constant sky
    samples = base[None] * (1.0 + sigma * rng.standard_normal((spp, h, w, 3))) if sigma else np.broadcast_to(base[None], (spp, h, w, 3))
    rgb = samples.mean(0)
    y = samples @ LUMA
    if spp >= 2:
        var = np.concatenate([samples.var(0, ddof=1), y.var(0, ddof=1)[..., None]], -1) / spp
    else:
        var = np.full((h, w, 4), np.inf)
    return rgb.astype(np.float32), gb.astype(np.float32), var.astype(np.float32)


# ------------------------------------------------------------------ the restatement
def reference(rgb, gb, var, cam, origin=(0, 0), prev=None, **params):
    """Steps 1 to 5 of the header in float64.  prev = (previous pinhole camera, previous gb12, previous history [H, W, 8]) or None.
    Returns (history [H, W, 8], rgb, var4, fragile [H, W] bool)."""
    P = dict(DEFAULTS, **params)
    rgb, gb, var = (np.asarray(a, np.float32).astype(np.float64) for a in (rgb, gb, var))
    f32 = lambda v: float(np.float32(v))
    alpha_min, normal_tol, plane_tol, eps, albedo_tol = (f32(P[k]) for k in ("alpha_min", "normal_tol", "plane_tol", "albedo_eps", "albedo_tol"))
    h, w = rgb.shape[:2]
    cov = gb[..., 10] > 0
    demod = cov & bool(P["flags"] & DEMODULATE)
    a = gb[..., 0:3]
    d = np.where(demod[..., None], np.where(a > eps, a, eps), 1.0)
    with np.errstate(all="ignore"):
        u_cur = rgb / d
        nu_cur = np.concatenate([var[..., :3] / (d * d), var[..., 3:4]], -1)
        passes = ~np.isfinite(u_cur).all(-1) | ~(nu_cur >= 0).all(-1)
    fragile = np.zeros((h, w), bool)
    W = np.zeros((h, w))
    acc = np.zeros((h, w, 8))
    if prev is not None:
        pcam, pgb, phist = prev
        same_view = all(np.array_equal(cam[k], pcam[k]) for k in ("c2w", "w2c", "r2c", "c2r"))    # equal cameras: no geometry tests
        pgb, phist = (np.asarray(x, np.float32).astype(np.float64) for x in (pgb, phist))
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
        v = np.where(cov[..., None], gb[..., 6:9], pixel_directions(cam, h, w, origin))
        with np.errstate(all="ignore"):
            cx, cy, _ = project(cam, v, cov)
            qx, qy, qz = project(pcam, v, cov)
            sx, sy = xs + (qx - cx), ys + (qy - cy)
            ok = (qz > 0) & (sx > -1) & (sx < w) & (sy > -1) & (sy < h)
            scale = np.abs(v).max(-1) + 1.0
            fragile |= np.abs(qz) < 1e-4 * scale
            for s, hi in (() if same_view else ((sx, w), (sy, h))):        # (equal cameras: the motion is exactly zero in any precision)
                fragile |= (np.abs(s + 1) < 1e-3) | (np.abs(s - hi) < 1e-3) | (np.abs(s - np.rint(s)) < 1e-4)
        sx, sy = np.where(ok, sx, 0.0), np.where(ok, sy, 0.0)
        ix, iy = np.floor(sx), np.floor(sy)
        tx, ty = sx - ix, sy - iy
        zc = np.maximum(gb[..., 9], 1e-6)
        n_p, x_p = gb[..., 3:6], gb[..., 6:9]
        for j in (0, 1):
            for i in (0, 1):
                b = (tx if i else 1 - tx) * (ty if j else 1 - ty)
                tqx, tqy = (ix + i).astype(np.int64), (iy + j).astype(np.int64)
                inside = ok & (b != 0) & (tqx >= 0) & (tqx < w) & (tqy >= 0) & (tqy < h)
                tqx, tqy = np.clip(tqx, 0, w - 1), np.clip(tqy, 0, h - 1)
                hq, gq = phist[tqy, tqx].copy(), pgb[tqy, tqx]
                with np.errstate(all="ignore"):
                    dq = np.where(gq[..., 0:3] > eps, gq[..., 0:3], eps)
                    big = np.maximum(d, dq)
                    convert = demod[..., None] & ~(np.abs(d - dq) <= albedo_tol * big)
                    near_d = (demod[..., None] & (np.abs(np.abs(d - dq) - albedo_tol * big) <= 1e-4 * np.maximum(albedo_tol * big, 1e-6))).any(-1)
                    hq[..., 0:3] = np.where(convert, hq[..., 0:3] * dq / d, hq[..., 0:3])
                    hq[..., 4:7] = np.where(convert, hq[..., 4:7] * (dq * dq) / (d * d), hq[..., 4:7])
                    fragile |= inside & (hq[..., 3] > 0) & ((gq[..., 10] > 0) == cov) & near_d
                    usable = (hq[..., 3] > 0) & np.isfinite(hq[..., :3]).all(-1) & ~np.isnan(hq[..., 4:]).any(-1)
                    count = inside & usable & ((gq[..., 10] > 0) == cov)
                    dn = ((n_p - gq[..., 3:6]) ** 2).sum(-1)
                    pd = np.abs((n_p * (x_p - gq[..., 6:9])).sum(-1))
                    geo = (dn <= normal_tol) & (pd <= plane_tol * zc)
                    near = (np.abs(dn - normal_tol) <= 1e-4 * max(normal_tol, 1e-6)) | (np.abs(pd - plane_tol * zc) <= 1e-4 * np.maximum(plane_tol * zc, 1e-6))
                if not same_view:
                    fragile |= count & cov & near
                    count &= geo | ~cov
                bb = np.where(count, b, 0.0)
                W += bb
                with np.errstate(all="ignore"):
                    acc += np.where(count[..., None], bb[..., None] * hq, 0.0)
        fragile |= (W > 0) & (W < W_FRAGILE)
    has = W > 0
    with np.errstate(all="ignore"):
        prev_v = acc / np.where(has, W, 1.0)[..., None]
        n1 = prev_v[..., 3] + 1.0
        alpha = np.maximum(1.0 / n1, alpha_min)
        blend = has & (alpha < 1.0)
        k = 1.0 - alpha
        u = np.where(blend[..., None], k[..., None] * prev_v[..., :3] + alpha[..., None] * u_cur, u_cur)
        nu = np.where(blend[..., None], (k * k)[..., None] * prev_v[..., 4:] + (alpha * alpha)[..., None] * nu_cur, nu_cur)
        n = np.where(blend, n1, 1.0)
        out_rgb = u * d
        out_var = np.concatenate([nu[..., :3] * (d * d), nu[..., 3:4]], -1)
    hist = np.concatenate([u, n[..., None], nu], -1)
    hist[passes] = 0.0
    out_rgb[passes] = rgb[passes]
    out_var[passes] = var[passes]
    fragile &= ~passes
    return hist, out_rgb, out_var, fragile


def rel_error(got, want):
    """max over the finite entries of |got - want| / max(|want|, 1e-3); non-finite entries must agree in kind"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)), "finite entries differ"
    assert np.array_equal(np.isnan(want), np.isnan(got)) and np.array_equal(want[~fin & ~np.isnan(want)], got[~fin & ~np.isnan(want)])
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-3)).max())
