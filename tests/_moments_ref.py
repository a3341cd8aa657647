"""A reference for the second moments (include/fountain_hip_moments.h) and per-tile adaptive sampling (include/fountain_hip_adaptive.h)
built from the CPU oracle's radiance of every camera sample (orc_render_sample_log), shared by test_moments_cpu.py, test_moments_oracle.py
and test_adaptive_abi.py.

The oracle reproduces the wavefront pipeline's radiance bit for bit, so a record's L is exactly what k_mo_accumulate squares.  From the
records this module rebuilds, in float32 and in the stated orders:
  oracle_film     orc_render's film: per-tile FilmTile sums in record order, merged in tile order (film.rs:95-172)
  gpu_sums        the beauty and the four moment sums in the moments header's order: a pixel's own samples from +0 in sample order, the
                  samples of other pixels of the same tile and of other tiles in two separate sums, then (own + in-tile) + other-tile;
                  plus what a bound on the GPU's atomically reordered spill sums needs
  keep_counts     the records a mixed-count render keeps: s < the count of the tile of the sample's own pixel
  simulate        the adaptive schedule, with the header's criterion (criterion_ref) applied to the sums the call would return
  variance64      the exact unbiased variance of each pixel's mean, in float64
  resolve_bound   a first-order bound on ftn_moments_resolve's one-pass float32 formula against that float64 variance"""
import ctypes as C

import numpy as np

from fountain_amd import Film, _abi as A

import _gbuffer_ref as GR

F32 = np.float32
U = 2.0 ** -24                     # unit roundoff of binary32
bits = GR.bits

RECORD = np.dtype([("px", "<i4"), ("py", "<i4"), ("sample", "<u4"), ("tile", "<u4"), ("p_film", "<f4", (2,)), ("L", "<f4", (3,)),
                   ("ray_weight", "<f4")])
assert RECORD.itemsize == 40

# ftn_math.h's conversions (float32 coefficients)
RGB2XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], F32)
XYZ2RGB = np.array([[3.240479, -1.537150, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]], F32)


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


def rgb_to_xyz(c):
    """ftn_math.h's rgb_to_xyz in float32: (a r + b g) + c b, no fused multiply-add"""
    c = np.asarray(c, F32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    return np.stack([((RGB2XYZ[k, 0] * r).astype(F32) + (RGB2XYZ[k, 1] * g).astype(F32)).astype(F32) + (RGB2XYZ[k, 2] * b).astype(F32)
                     for k in range(3)], -1).astype(F32)


# ------------------------------------------------------------------ the records
def sample_log(orc, scene, cam, film, integrator, sampler, tiles=None, n_threads=16):
    """orc_render_sample_log: (records [n] RECORD, stats)"""
    tr = A.ftn_tile_range()
    tr.first, tr.stride, tr.count = tiles if tiles is not None else (0, 1, 0)
    fn = orc.lib.orc_render_sample_log
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    args = [scene.handle, C.byref(cam.desc), C.byref(film.desc), C.byref(sampler.desc), C.byref(integrator.desc), C.byref(tr), n_threads]
    n = C.c_size_t()
    orc.check(fn(*args, None, 0, C.byref(n), None, None))
    rec = np.zeros(n.value, RECORD)
    st = A.ftn_stats()
    orc.check(fn(*args, rec.ctypes.data_as(C.c_void_p), C.c_size_t(n.value), C.byref(n), None, C.byref(st)))
    assert n.value == len(rec)
    return rec, st.as_dict()


def oracle_records(orc, make, integrator, sampler, crop=(0.0, 0.0, 1.0, 1.0), radius=(0.5, 0.5), tiles=None):
    """the scene `make(be) -> (builder, camera, res)` on the oracle: (records, film, stats)"""
    b, cam, res = make(orc)
    sc = b.create_scene()
    f = GR.film(orc, res, crop, radius)
    rec, st = sample_log(orc, sc, cam, f, integrator, sampler, tiles)
    return rec, f, st


# ------------------------------------------------------------------ footprints
def entries(film, sel, rec):
    """every (record, pixel) pair a record's box-filter footprint touches, clipped to its tile's get_film_tile bounds (GR.footprint,
    vectorised), in record order.  Returns (record index, x, y, kind) with kind 0 = the record's own pixel, 1 = another pixel of its
    tile, 2 = a pixel of another tile, and the number of pixels each record touched."""
    rx, ry = F32(film.desc.filter_radius[0]), F32(film.desc.filter_radius[1])
    tpb = np.array([GR.tile_pixel_bounds(film, t) for t in sel], np.int64).reshape(-1, 4)[rec["tile"]]
    sb = np.array(sel, np.int64).reshape(-1, 4)[rec["tile"]]
    pdx = (rec["p_film"][:, 0] - F32(0.5)).astype(F32)
    pdy = (rec["p_film"][:, 1] - F32(0.5)).astype(F32)
    x0 = np.maximum(np.ceil((pdx - rx).astype(F32)).astype(np.int64), tpb[:, 0])
    y0 = np.maximum(np.ceil((pdy - ry).astype(F32)).astype(np.int64), tpb[:, 1])
    x1 = np.minimum(np.floor((pdx + rx).astype(F32)).astype(np.int64) + 1, tpb[:, 2])
    y1 = np.minimum(np.floor((pdy + ry).astype(F32)).astype(np.int64) + 1, tpb[:, 3])
    nx, ny = np.maximum(x1 - x0, 0), np.maximum(y1 - y0, 0)
    parts = []
    for dy in range(int(ny.max()) if len(rec) else 0):
        for dx in range(int(nx.max())):
            i = np.nonzero((dx < nx) & (dy < ny))[0]
            parts.append((i, x0[i] + dx, y0[i] + dy))
    if not parts:
        z = np.zeros(0, np.int64)
        return z, z, z, z, nx * ny
    i, x, y = (np.concatenate([p[k] for p in parts]) for k in range(3))
    order = np.argsort(i, kind="stable")
    i, x, y = i[order], x[order], y[order]
    own = (x == rec["px"][i]) & (y == rec["py"][i])
    in_tile = (x >= sb[i, 0]) & (x < sb[i, 2]) & (y >= sb[i, 1]) & (y < sb[i, 3])
    kind = np.where(own, 0, np.where(in_tile, 1, 2))
    return i, x, y, kind, nx * ny


def _squares(L):
    """the four values k_mo_accumulate adds per sample: L.r^2, L.g^2, L.b^2, Y^2 (float32)"""
    y = rgb_to_xyz(L)[:, 1]
    return np.stack([L[:, 0] * L[:, 0], L[:, 1] * L[:, 1], L[:, 2] * L[:, 2], y * y], -1).astype(F32)


# ------------------------------------------------------------------ orc_render's film
def oracle_film(film, sel, rec):
    """orc_render's pixels from its own records: each tile's FilmTile sums its records' contrib = L * ray_weight * 1 in record order,
    and merge_film_tile adds rgb_to_xyz of every tile pixel into the film in tile order (from a zero film)"""
    c = film.desc.crop
    W = film.width
    tpb = [GR.tile_pixel_bounds(film, t) for t in sel]
    dims = [(max(b[2] - b[0], 0), max(b[3] - b[1], 0)) for b in tpb]
    off = np.concatenate([[0], np.cumsum([w * h for w, h in dims])]).astype(np.int64)
    i, x, y, _, _ = entries(film, sel, rec)
    k = rec["tile"][i].astype(np.int64)
    b = np.array(tpb, np.int64).reshape(-1, 4)
    wk = np.array([d[0] for d in dims], np.int64)
    slot = off[k] + (y - b[k, 1]) * wk[k] + (x - b[k, 0])
    contrib = ((rec["L"][i] * rec["ray_weight"][i, None]).astype(F32) * F32(1.0)).astype(F32)
    tile_rgb = np.zeros((off[-1], 3), F32)
    tile_w = np.zeros(off[-1], F32)
    np.add.at(tile_rgb, slot, contrib)
    np.add.at(tile_w, slot, F32(1.0))
    # the merge: tile order, then the tile's pixel bounds (every pixel once per tile)
    pix_of_slot = np.concatenate([((yy - c[1]) * W + (xx - c[0])).ravel()
                                  for (x0, y0, x1, y1) in tpb for yy, xx in [np.mgrid[y0:max(y1, y0), x0:max(x1, x0)]]]).astype(np.int64)
    out = np.zeros((film.height * film.width, 4), F32)
    np.add.at(out, pix_of_slot, np.concatenate([rgb_to_xyz(tile_rgb), tile_w[:, None]], -1))
    return out.reshape(film.height, film.width, 4)


# ------------------------------------------------------------------ the moments header's sums
def gpu_sums(film, sel, rec):
    """The beauty (ftn_pixel) and moments (ftn_moment_pixel) a moments call writes into zero buffers, in the header's order, and per pixel:
    foreign (a sample of another pixel landed), terms (samples summed), mag_rgb / mag_sq (sums of the magnitudes of the beauty's and the
    moments' terms, float64), n (camera samples), n_spill (samples that did not touch exactly one pixel)."""
    H, W = film.height, film.width
    c = film.desc.crop
    i, x, y, kind, touched = entries(film, sel, rec)
    p = (y - c[1]) * W + (x - c[0])
    L = rec["L"][i]
    contrib = ((L * rec["ray_weight"][i, None]).astype(F32) * F32(1.0)).astype(F32)
    q = _squares(L)
    acc = np.zeros((3, H * W, 4), F32)                    # own, in-tile, other-tile: rgb + weight
    mom = np.zeros((3, H * W, 4), F32)
    for k in range(3):
        m = kind == k
        np.add.at(acc[k], p[m], np.concatenate([contrib[m], np.ones((int(m.sum()), 1), F32)], -1))
        np.add.at(mom[k], p[m], q[m])
    a, b, cc = acc
    beauty = np.zeros((H * W, 4), F32)
    beauty[:, :3] = F32(0) + rgb_to_xyz((a[:, :3] + b[:, :3]).astype(F32))
    beauty[:, 3] = F32(0) + (a[:, 3] + b[:, 3]).astype(F32)
    spill = cc[:, 3] != 0
    beauty[spill, :3] = (beauty[spill, :3] + rgb_to_xyz(cc[spill, :3])).astype(F32)
    beauty[spill, 3] = (beauty[spill, 3] + cc[spill, 3]).astype(F32)
    moments = ((F32(0) + (mom[0] + mom[1]).astype(F32)) + mom[2]).astype(F32)
    foreign = np.zeros(H * W, bool)
    foreign[p[kind != 0]] = True
    terms = np.bincount(p, minlength=H * W)
    mag_rgb = np.zeros((H * W, 3), np.float64)
    mag_sq = np.zeros((H * W, 4), np.float64)
    np.add.at(mag_rgb, p, np.abs(contrib.astype(np.float64)))
    np.add.at(mag_sq, p, q.astype(np.float64))
    sh = (H, W)
    return dict(beauty=beauty.reshape(sh + (4,)), moments=moments.reshape(sh + (4,)), foreign=foreign.reshape(sh), terms=terms.reshape(sh),
                mag_rgb=mag_rgb.reshape(sh + (3,)), mag_sq=mag_sq.reshape(sh + (4,)), n=len(rec), n_spill=int((touched != 1).sum()),
                p=p, i=i)


def spill_bounds(ref):
    """per pixel, how far a float32 sum of the same terms in another order may lie from the reference's: the moments within
    2 gamma(n) sum|x| (n terms); the beauty's xyz within the same bound of its rgb sums pushed through |RGB2XYZ|, plus the conversions
    and the final add (gamma(n + 4) in all)"""
    n = ref["terms"][..., None].astype(np.float64)
    b_mom = 2.0 * gamma(n) * ref["mag_sq"]
    b_xyz = 2.0 * gamma(n + 4) * (ref["mag_rgb"] @ np.abs(RGB2XYZ.astype(np.float64)).T)
    return b_xyz, b_mom


def assert_matches(got_px, got_m, ref, what=""):
    """weights bit-equal everywhere; the beauty's xyz and all four moments bit-equal where no sample of another pixel landed, within
    the reordering bound where one did"""
    want_px, want_m, foreign = ref["beauty"], ref["moments"], ref["foreign"]
    assert np.array_equal(bits(got_px[..., 3]), bits(want_px[..., 3])), "%s: weights differ at %d pixels" % (
        what, int((bits(got_px[..., 3]) != bits(want_px[..., 3])).sum()))
    for name, got, want in (("beauty", got_px[..., :3], want_px[..., :3]), ("moments", got_m, want_m)):
        diff = (bits(got) != bits(want)).any(-1) & ~foreign
        assert not diff.any(), "%s: %s differ at %d pixels where no foreign sample landed, first %r channel %r: %r vs %r" % (
            what, name, int(diff.sum()), tuple(np.argwhere(diff)[0]), np.nonzero(bits(got)[tuple(np.argwhere(diff)[0])] != bits(want)[tuple(np.argwhere(diff)[0])])[0],
            got[tuple(np.argwhere(diff)[0])], want[tuple(np.argwhere(diff)[0])])
    b_xyz, b_mom = spill_bounds(ref)
    for name, got, want, bound in (("beauty", got_px[..., :3], want_px[..., :3], b_xyz), ("moments", got_m, want_m, b_mom)):
        err = np.abs(got.astype(np.float64) - want)
        over = err > bound
        assert not over.any(), "%s: %s: %d spill values beyond the reordering bound, first %r (err %.3g, bound %.3g)" % (
            what, name, int(over.sum()), tuple(np.argwhere(over)[0]), err[over][0], bound[over][0])


# ------------------------------------------------------------------ mixed counts
def keep_counts(rec, counts):
    """the records a call that ends tile k at counts[k] keeps: s < the count of the tile of the sample's own pixel"""
    return rec[rec["sample"] < np.asarray(counts, np.int64)[rec["tile"]]]


# ------------------------------------------------------------------ the adaptive criterion and schedule
def criterion_ref(pix, m, t, a):
    """the header's criterion in float32, one rounding per step: v = Y of the moments resolve (W < 2 -> inf); mean = Y / W; t2 = t * t;
    a2 = a * a; bound = t2 * (mean * mean + a2); converged iff Y, W, sq_y, v and bound are finite and v <= bound"""
    pix, m = np.asarray(pix, F32), np.asarray(m, F32)
    y, w = pix[..., 1], pix[..., 3]
    t, a = F32(t), F32(a)
    with np.errstate(all="ignore"):
        mean = (y / w).astype(F32)
        v = ((m[..., 3] / w).astype(F32) - (mean * mean).astype(F32)).astype(F32)
        v = np.where(v < 0, F32(0), v).astype(F32)
        v = (v / (w - F32(1))).astype(F32)
        v = np.where(w < 2, F32(np.inf), v)
        t2, a2 = F32(t * t), F32(a * a)
        bound = (t2 * (mean * mean + a2).astype(F32)).astype(F32)
        fin = np.isfinite(y) & np.isfinite(w) & np.isfinite(m[..., 3]) & np.isfinite(v) & np.isfinite(bound)
        return (fin & (v <= bound)).astype(np.uint8)


def schedule(n0, N, step):
    """the header's rounds: n0, then n_{r+1} = min(N, n_r + (step or n_r))"""
    s = [n0]
    while s[-1] < N:
        s.append(min(N, s[-1] + (step or s[-1])))
    return s


def spill_window(ref, t, a):
    """per pixel, the relative change of t under which the criterion's verdict is sure in spite of the spill sums' reordering: how far
    that bound can move v and B, against B, first order (each float32 step adds at most u of its operands)"""
    b_xyz, b_mom = spill_bounds(ref)
    px, m = ref["beauty"].astype(np.float64), ref["moments"].astype(np.float64)
    w = px[..., 3]
    with np.errstate(all="ignore"):
        mean = np.abs(px[..., 1]) / w
        dmean = b_xyz[..., 1] / w
        q = m[..., 3] / w
        dv = (b_mom[..., 3] / w + 2 * mean * dmean + dmean * dmean + 6 * U * (q + mean * mean)) / (w - 1)
        B = float(t) ** 2 * (mean * mean + float(a) ** 2)
        dB = float(t) ** 2 * (2 * mean * dmean + dmean * dmean) + 6 * U * B
        out = np.where(ref["foreign"] & (w >= 2), (dv + dB) / B, 0.0)
    return np.where(np.isfinite(out), out, np.inf)


def tile_slices(film, sel):
    """per selected tile, its crop pixels as (row slice, column slice)"""
    c = film.desc.crop
    out = []
    for (x0, y0, x1, y1) in sel:
        out.append((slice(max(y0, c[1]) - c[1], max(min(y1, c[3]) - c[1], 0)), slice(max(x0, c[0]) - c[0], max(min(x1, c[2]) - c[0], 0))))
    return out


def simulate(film, sel, rec, N, n0, step, t, a, window=1e-3):
    """The adaptive schedule from the records.  Round r renders [n_{r-1}, n_r) for the active tiles; after it, every active tile's pixels
    get the sums the call would return now (gpu_sums of the records kept so far: adaptive_pixel_sums), and a tile stops when every one of
    its crop pixels passes criterion_ref.  A tile is unsure at a round when its verdict differs between t (1 - w) and t (1 + w), with w
    the larger of `window` and the pixel's spill_window.  Returns dict(counts [tiles], rounds, unsure [tiles], unsure_rounds)."""
    sched = schedule(n0, N, step)
    n_t = len(sel)
    counts = np.zeros(n_t, np.int64)
    active = np.ones(n_t, bool)
    unsure = np.zeros(n_t, bool)
    slices = tile_slices(film, sel)
    rounds = 0
    for n in sched:
        if not active.any():
            break
        rounds += 1
        counts[active] = n
        if n >= N:
            break
        ref = gpu_sums(film, sel, keep_counts(rec, counts))
        w = np.maximum(window, spill_window(ref, t, a))
        lo, mid, hi = (criterion_ref(ref["beauty"], ref["moments"], (F32(t) * (1.0 + s * w)).astype(F32), a) for s in (-1, 0, 1))
        for k in np.nonzero(active)[0]:
            ys, xs = slices[k]
            v_lo, v_mid, v_hi = bool(lo[ys, xs].all()), bool(mid[ys, xs].all()), bool(hi[ys, xs].all())
            if v_lo != v_hi:
                unsure[k] = True
            if v_mid:
                active[k] = False
    return dict(counts=counts, rounds=rounds, unsure=unsure)


def per_pixel(film, sel, per_tile, fill=0):
    """a per-tile array spread over the crop pixels of each tile (fill elsewhere)"""
    out = np.full((film.height, film.width), fill, np.asarray(per_tile).dtype)
    for k, (ys, xs) in enumerate(tile_slices(film, sel)):
        out[ys, xs] = per_tile[k]
    return out


# ------------------------------------------------------------------ float64 variance and the resolve's bound
def variance64(film, ref, rec):
    """the exact unbiased variance of each pixel's mean for r, g, b (raw radiance L) and Y (the float32 Y each sample squares), in
    float64 and two passes over the samples that touched the pixel (box filter: weight 1).  Returns (var [H, W, 4], mean [H, W, 4],
    sum|x| [H, W, 4], W [H, W]); inf where W < 2."""
    H, Wd = film.height, film.width
    p, i = ref["p"], ref["i"]
    L = rec["L"][i].astype(np.float64)
    x = np.concatenate([L, rgb_to_xyz(rec["L"][i])[:, 1:2].astype(np.float64)], -1)
    w = np.bincount(p, minlength=H * Wd).astype(np.float64)
    s = np.zeros((H * Wd, 4))
    np.add.at(s, p, x)
    with np.errstate(all="ignore"):
        mean = s / w[:, None]
        d = np.zeros((H * Wd, 4))
        np.add.at(d, p, (x - mean[p]) ** 2)
        var = d / (w * (w - 1))[:, None]
    var[w < 2] = np.inf
    absx = np.zeros((H * Wd, 4))
    np.add.at(absx, p, np.abs(x))
    sh = (H, Wd)
    return var.reshape(sh + (4,)), mean.reshape(sh + (4,)), absx.reshape(sh + (4,)), w.reshape(sh)


def resolve_bound(px, m, absx, absL, absq):
    """A first-order bound on |ftn_moments_resolve(px, m) - the float64 variance of the mean|, from the header's steps, per channel.
    px, m: the float32 sums the resolve reads; absx: per pixel and channel sum|x| of the terms (r, g, b, Y); absL: sum|L| per rgb
    channel; absq: sum of the squares.  Errors of the inputs against the exact sums: e_S (the beauty stores rgb_to_xyz of float32 rgb
    sums, which the resolve turns back with xyz_to_rgb, whose coefficients invert RGB2XYZ only to about 1e-6), e_sq (float32 sums of
    float32 squares).  Then mean = S / W, q = sq / W, p = mean * mean, d = q - p, clamp, d / (W - 1), each one rounding:
    |out - v| <= (|dq| + |dp| + u |q - p|) / (W - 1) + u |out|, |dq| <= e_sq / W + u q, |dp| <= (2 |m| + dm) dm + u p,
    dm <= e_S / W + u |mean|."""
    px, m = np.asarray(px, np.float64), np.asarray(m, np.float64)
    W = px[..., 3]
    n = W[..., None]
    Mi, Mf = XYZ2RGB.astype(np.float64), RGB2XYZ.astype(np.float64)
    E = np.abs(Mi @ Mf - np.eye(3))
    absMiMf = np.abs(Mi) @ np.abs(Mf)
    e_S = np.empty(px.shape)
    e_S[..., :3] = absL @ E.T + gamma(n + 8) * (absL @ absMiMf.T)
    e_S[..., 3] = (gamma(W + 8) * (absL @ np.abs(Mf[1])))
    S = np.empty(px.shape)
    with np.errstate(all="ignore"):
        S[..., :3] = px[..., :3] @ Mi.T
        S[..., 3] = px[..., 1]
        e_sq = gamma(n + 1) * absq
        mean = np.abs(S) / n
        dm = e_S / n + U * mean
        q = m / n
        dq = e_sq / n + U * q
        p = mean * mean
        dp = (2 * mean + dm) * dm + U * p
        out = (dq + dp + U * np.abs(q - p)) / (n - 1)
        out = out * (1 + 4 * U) + U * np.abs(q - p) / (n - 1)
    return out
