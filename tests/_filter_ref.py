"""An independent restatement of the reconstruction-filtered film (include/fountain_hip_filter.h) in numpy, shared by test_filter_abi.py,
test_filter_cpu.py and test_filter.py.  Nothing here calls the library's filter code:

  table64        Film::new's table from PBRT v3's filter definitions, in float64
  film_ref       the header's footprint, weight, term and order rules over a list of camera samples, in float32 (np.add.at adds in index
                 order, one rounding per add), with what the bounds need: float64 sums, term counts and sums of magnitudes
  sum_bound      the bound of a float32 sum of n terms pushed through rgb_to_xyz against its float64 value

The sample records are _moments_ref.RECORD arrays (orc_render_sample_log)."""
import numpy as np

import _moments_ref as MR

F32 = np.float32
U = MR.U
KINDS = ("box", "triangle", "gaussian", "mitchell", "sinc")
DEFAULTS = {"box": (0.5, ()), "triangle": (2.0, ()), "gaussian": (2.0, (2.0,)), "mitchell": (2.0, (1.0 / 3.0, 1.0 / 3.0)), "sinc": (4.0, (3.0,))}


def _mitchell(v, B, C):
    t = np.abs(2.0 * v)
    far = ((-B - 6 * C) * t * t * t + (6 * B + 30 * C) * t * t + (-12 * B - 48 * C) * t + (8 * B + 24 * C)) * (1.0 / 6.0)
    near = ((12 - 9 * B - 6 * C) * t * t * t + (-18 + 12 * B + 6 * C) * t * t + (6 - 2 * B)) * (1.0 / 6.0)
    return np.where(t > 1, far, near)


def _sinc(v):
    v = np.abs(v)
    safe = np.where(v < 1e-5, 1.0, v)
    return np.where(v < 1e-5, 1.0, np.sin(np.pi * safe) / (np.pi * safe))


def evaluate64(kind, rx, ry, params, x, y):
    """PBRT v3's Filter::Evaluate in float64; rx, ry and params are the float32 values of the description"""
    rx, ry = float(F32(rx)), float(F32(ry))
    p = [float(F32(v)) for v in params]
    if kind == "box":
        return np.ones(np.broadcast(x, y).shape)
    if kind == "triangle":
        return np.maximum(0.0, rx - np.abs(x)) * np.maximum(0.0, ry - np.abs(y))
    if kind == "gaussian":
        g = lambda v, r: np.maximum(0.0, np.exp(-p[0] * v * v) - np.exp(-p[0] * r * r))
        return g(x, rx) * g(y, ry)
    if kind == "mitchell":
        return _mitchell(x / rx, p[0], p[1]) * _mitchell(y / ry, p[0], p[1])
    l = lambda v, r: np.where(np.abs(v) > r, 0.0, _sinc(v) * _sinc(v / p[0]))
    return l(x, rx) * l(y, ry)


def table64(kind, rx, ry, params):
    """entry [y][x] = evaluate((x + 0.5) rx / 16, (y + 0.5) ry / 16), float64"""
    k = np.arange(16) + 0.5
    return evaluate64(kind, rx, ry, params, (k * float(F32(rx)) / 16.0)[None, :], (k * float(F32(ry)) / 16.0)[:, None])


def film_ref(film, table, rec):
    """The filtered film of the records `rec` into a zero buffer.  table: [16, 16] float32.  Returns dict(pixels [H, W, 4] float32 ftn_pixel,
    xyz64 / w64: the same sums in float64 (the float32 terms' factors, exact products), terms [H, W], mag [H, W, 3] = sum |w L| per rgb
    channel, magw [H, W] = sum |w|, w1 / w2 [H, W] = sum w, sum w^2 (float64))."""
    H, W = film.height, film.width
    c = list(film.desc.crop)
    rx, ry = F32(film.desc.filter_radius[0]), F32(film.desc.filter_radius[1])
    inv_rx, inv_ry = F32(1.0) / rx, F32(1.0) / ry
    table = np.asarray(table, F32).reshape(16, 16)
    rec = rec[np.lexsort((rec["px"], rec["py"], rec["sample"]))]                    # (sample, py, px)
    pdx = (rec["p_film"][:, 0] - F32(0.5)).astype(F32)
    pdy = (rec["p_film"][:, 1] - F32(0.5)).astype(F32)
    x0 = np.maximum(np.ceil((pdx - rx).astype(F32)).astype(np.int64), c[0])
    y0 = np.maximum(np.ceil((pdy - ry).astype(F32)).astype(np.int64), c[1])
    x1 = np.minimum(np.floor((pdx + rx).astype(F32)).astype(np.int64), c[2] - 1)       # inclusive
    y1 = np.minimum(np.floor((pdy + ry).astype(F32)).astype(np.int64), c[3] - 1)
    nx, ny = np.maximum(x1 - x0 + 1, 0), np.maximum(y1 - y0 + 1, 0)
    parts = []
    for dy in range(int(ny.max()) if len(rec) else 0):
        for dx in range(int(nx.max())):
            i = np.nonzero((dx < nx) & (dy < ny))[0]
            parts.append((i, x0[i] + dx, y0[i] + dy))
    out = dict(pixels=np.zeros((H, W, 4), F32), xyz64=np.zeros((H, W, 3)), w64=np.zeros((H, W)), terms=np.zeros((H, W), np.int64),
               mag=np.zeros((H, W, 3)), magw=np.zeros((H, W)), w1=np.zeros((H, W)), w2=np.zeros((H, W)))
    if not parts:
        return out
    i, x, y = (np.concatenate([p[k] for p in parts]) for k in range(3))
    order = np.argsort(i, kind="stable")            # a pixel meets each record at most once: record order is the pixel's term order
    i, x, y = i[order], x[order], y[order]
    ix = np.minimum(np.floor(np.abs(((x.astype(F32) - pdx[i]).astype(F32) * inv_rx).astype(F32) * F32(16.0)).astype(F32)).astype(np.int64), 15)
    iy = np.minimum(np.floor(np.abs(((y.astype(F32) - pdy[i]).astype(F32) * inv_ry).astype(F32) * F32(16.0)).astype(F32)).astype(np.int64), 15)
    w = table[iy, ix]
    L = (rec["L"][i] * F32(1.0)).astype(F32)
    term = (L * w[:, None]).astype(F32)
    p = (y - c[1]) * W + (x - c[0])
    acc = np.zeros((H * W, 4), F32)
    with np.errstate(all="ignore"):
        np.add.at(acc, p, np.concatenate([term, w[:, None]], -1))
        px = np.zeros((H * W, 4), F32)
        px[:, :3] = F32(0) + (F32(0) + MR.rgb_to_xyz(acc[:, :3]))
        px[:, 3] = F32(0) + (F32(0) + acc[:, 3])
    w_d, L_d = w.astype(np.float64), L.astype(np.float64)
    rgb64 = np.zeros((H * W, 3)); np.add.at(rgb64, p, L_d * w_d[:, None])
    mag = np.zeros((H * W, 3)); np.add.at(mag, p, np.abs(L_d * w_d[:, None]))
    out["pixels"] = px.reshape(H, W, 4)
    out["xyz64"] = (rgb64 @ MR.RGB2XYZ.astype(np.float64).T).reshape(H, W, 3)
    out["w64"] = np.bincount(p, w_d, H * W).reshape(H, W)
    out["terms"] = np.bincount(p, minlength=H * W).reshape(H, W)
    out["mag"] = mag.reshape(H, W, 3)
    out["magw"] = np.bincount(p, np.abs(w_d), H * W).reshape(H, W)
    out["w1"] = out["w64"]
    out["w2"] = np.bincount(p, w_d * w_d, H * W).reshape(H, W)
    return out


def sum_bound(ref, factor=1.0):
    """|float32 film - float64 sums| per pixel, [H, W, 4]: a term fl(L w) carries one rounding and at most n - 1 additions follow it, and
    rgb_to_xyz's (a r + b g) + c b adds at most three more: gamma(n + 3) sum |w L| through |RGB2XYZ| for xyz, gamma(n + 3) sum |w| for the
    weight (it has no product and no conversion: the same bound is generous)."""
    g = MR.gamma(ref["terms"] + 3.0)[..., None]
    b = np.concatenate([g * (ref["mag"] @ np.abs(MR.RGB2XYZ.astype(np.float64)).T), g * ref["magw"][..., None]], -1)
    return factor * b


def assert_within(got, ref, factor=1.0, what=""):
    want = np.concatenate([ref["xyz64"], ref["w64"][..., None]], -1)
    err = np.abs(got.astype(np.float64) - want)
    b = sum_bound(ref, factor)
    assert (err <= b).all(), "%s: %d values beyond the bound, worst ratio %.3g" % (what, int((err > b).sum()), float((err / np.maximum(b, 1e-300)).max()))


def desc_params(filt):
    """(kind name, rx, ry, params) of a fountain_amd.filters.Filter"""
    n = {"box": 0, "triangle": 0, "gaussian": 1, "mitchell": 2, "sinc": 1}[filt.kind]
    return filt.kind, filt.desc.radius[0], filt.desc.radius[1], tuple(filt.desc.param[k] for k in range(n))
