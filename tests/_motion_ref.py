"""A float64 numpy restatement of what include/fountain_hip_motion.h changes in temporal accumulation, and of ftn_motion_vectors, built
on tests/_temporal_ref.py (its cameras, frames, projection and fragility marks) and sharing no code with the library; synthetic frames of
a square that moves over a background plane, with analytic gb12 and mv8.

reference_motion() is _temporal_ref.reference() with the header's changes: a covered pixel projects its previous position into the
previous camera and its own into the current one, both tap tests use the previous position and normal, the equal-camera shortcut holds
per pixel and only where the previous values are the pixel's own bit for bit, and a pixel whose mv8 coverage class differs from gb12's
has no history.  mv8 = None is reference() itself.
"""
import numpy as np

import _temporal_ref as R


def mv8_from_gb(gb):
    """an mv8 whose position, normal, coverage and weight are copied from gb12: a scene in which nothing moved"""
    gb = np.asarray(gb, np.float32)
    return np.ascontiguousarray(np.concatenate([gb[..., 6:9], gb[..., 3:6], gb[..., 10:12]], -1))


def motion_vectors(mv8, gb, cam, pcam, origin=(0, 0)):
    """ftn_motion_vectors in float64: (motion [H, W, 2] with NaN where there is none, fragile [H, W]) -- fragile where a binary32 rounding
    may flip q.z > 0"""
    mv8, gb = (np.asarray(a, np.float32).astype(np.float64) for a in (mv8, gb))
    h, w = gb.shape[:2]
    cov = gb[..., 10] > 0
    D = R.pixel_directions(cam, h, w, origin)
    v_cur = np.where(cov[..., None], gb[..., 6:9], D)
    v_prev = np.where(cov[..., None], mv8[..., 0:3], D)
    with np.errstate(all="ignore"):
        cx, cy, _ = R.project(cam, v_cur, cov)
        qx, qy, qz = R.project(pcam, v_prev, cov)
        seen = (qz > 0) & ((mv8[..., 6] > 0) == cov)
        out = np.stack([np.where(seen, qx - cx, np.nan), np.where(seen, qy - cy, np.nan)], -1)
        fragile = np.abs(qz) < 1e-4 * (np.abs(v_prev).max(-1) + 1.0)
    return out, fragile


def reference_motion(rgb, gb, var, cam, mv8=None, origin=(0, 0), prev=None, **params):
    """Steps 1 to 5 in float64 with the frame's mv8.  Returns (history [H, W, 8], rgb, var4, fragile [H, W] bool)."""
    if mv8 is None:
        return R.reference(rgb, gb, var, cam, origin, prev, **params)
    P = dict(R.DEFAULTS, **params)
    rgb, gb, var = (np.asarray(a, np.float32).astype(np.float64) for a in (rgb, gb, var))
    mv32 = np.asarray(mv8, np.float32)
    mv = mv32.astype(np.float64)
    f32 = lambda v: float(np.float32(v))
    alpha_min, normal_tol, plane_tol, eps, albedo_tol = (f32(P[k]) for k in ("alpha_min", "normal_tol", "plane_tol", "albedo_eps", "albedo_tol"))
    h, w = rgb.shape[:2]
    cov = gb[..., 10] > 0
    demod = cov & bool(P["flags"] & R.DEMODULATE)
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
        same_view = all(np.array_equal(cam[k], pcam[k]) for k in ("c2w", "w2c", "r2c", "c2r"))
        gb32 = np.asarray(gb, np.float32)
        own = np.concatenate([gb32[..., 6:9], gb32[..., 3:6]], -1)
        still = (mv32[..., :6].view(np.uint32) == own.view(np.uint32)).all(-1) | ~cov        # bit for bit
        untested = same_view & still                                                           # per pixel
        same_class = (mv[..., 6] > 0) == cov
        pgb, phist = (np.asarray(x, np.float32).astype(np.float64) for x in (pgb, phist))
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
        D = R.pixel_directions(cam, h, w, origin)
        v_cur = np.where(cov[..., None], gb[..., 6:9], D)
        v_prev = np.where(cov[..., None], mv[..., 0:3], D)
        with np.errstate(all="ignore"):
            cx, cy, _ = R.project(cam, v_cur, cov)
            qx, qy, qz = R.project(pcam, v_prev, cov)
            sx, sy = xs + (qx - cx), ys + (qy - cy)
            ok = same_class & (qz > 0) & (sx > -1) & (sx < w) & (sy > -1) & (sy < h)
            scale = np.abs(v_prev).max(-1) + 1.0
            fragile |= np.abs(qz) < 1e-4 * scale
            same_point = (mv32[..., :3].view(np.uint32) == gb32[..., 6:9].view(np.uint32)).all(-1) | ~cov
            exact = same_view & same_point                 # the same function on the same input twice: a motion of exactly zero
            for s, hi in ((sx, w), (sy, h)):
                fragile |= ~exact & ((np.abs(s + 1) < 1e-3) | (np.abs(s - hi) < 1e-3) | (np.abs(s - np.rint(s)) < 1e-4))
        sx, sy = np.where(ok, sx, 0.0), np.where(ok, sy, 0.0)
        ix, iy = np.floor(sx), np.floor(sy)
        tx, ty = sx - ix, sy - iy
        zc = np.maximum(gb[..., 9], 1e-6)
        n_q, x_q = np.where(cov[..., None], mv[..., 3:6], gb[..., 3:6]), np.where(cov[..., None], mv[..., 0:3], gb[..., 6:9])
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
                    dn = ((n_q - gq[..., 3:6]) ** 2).sum(-1)
                    pd = np.abs((n_q * (x_q - gq[..., 6:9])).sum(-1))
                    geo = (dn <= normal_tol) & (pd <= plane_tol * zc)
                    near = (np.abs(dn - normal_tol) <= 1e-4 * max(normal_tol, 1e-6)) | (np.abs(pd - plane_tol * zc) <= 1e-4 * np.maximum(plane_tol * zc, 1e-6))
                tested = cov & ~untested
                fragile |= count & tested & near
                count &= geo | ~tested
                bb = np.where(count, b, 0.0)
                W += bb
                with np.errstate(all="ignore"):
                    acc += np.where(count[..., None], bb[..., None] * hq, 0.0)
        fragile |= (W > 0) & (W < R.W_FRAGILE)
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


# ------------------------------------------------------------------ a square that moves over a background plane
def moving_square_frame(cam, k, h, w, step=(0.09, 0.05), half=0.45, z_obj=2.0, z_bg=4.0, spp=4, sigma=0.3, seed=0, sky_until=-0.2):
    """Frame k: a textured square of half-width `half` on the plane z = z_obj, its centre at k * step, in front of a textured background
    plane z = z_bg that begins at x = sky_until (left of it: uncovered sky); the camera `cam` stands still.  The radiance samples are the
    surface's colour -- a function of the OBJECT's own coordinates on the square, of the world's on the background -- times noise of
    relative size sigma.  Returns (rgb, gb12, var4, mv8, clean rgb, object mask): mv8's previous position of an object pixel is its
    position minus step, of a background pixel its own; the normals do not change."""
    rng = np.random.default_rng(seed + 977 * k)
    D = R.pixel_directions(cam, h, w)
    eye = cam["eye"]
    centre = np.array([k * step[0], k * step[1]])
    t_obj, t_bg = (z_obj - eye[2]) / D[..., 2], (z_bg - eye[2]) / D[..., 2]
    X_obj, X_bg = eye + t_obj[..., None] * D, eye + t_bg[..., None] * D
    obj = (np.abs(X_obj[..., 0] - centre[0]) <= half) & (np.abs(X_obj[..., 1] - centre[1]) <= half)
    cov = obj | (X_bg[..., 0] >= sky_until)
    X = np.where(obj[..., None], X_obj, np.where(cov[..., None], X_bg, 0.0))
    local = X.copy()
    local[..., :2] -= np.where(obj[..., None], centre, 0.0)
    clean = np.where(cov[..., None], np.where(obj[..., None], R.texture(local, 4.0), 0.5 * R.texture(local, 0.7)), 0.3)
    gb = np.zeros((h, w, 12))
    nrm = np.zeros((h, w, 3))
    nrm[..., 2] = -1.0
    gb[..., 0:3], gb[..., 3:6], gb[..., 6:9], gb[..., 9], gb[..., 10] = R.albedo_of(local), nrm, X, R._point(cam["w2c"], X)[..., 2], 1.0
    gb[~cov] = 0.0
    gb[..., 11] = spp
    samples = clean[None] * (1.0 + sigma * rng.standard_normal((spp, h, w, 3)))
    rgb = samples.mean(0)
    var = np.concatenate([samples.var(0, ddof=1), (samples @ R.LUMA).var(0, ddof=1)[..., None]], -1) / spp
    gb32 = gb.astype(np.float32)
    mv = mv8_from_gb(gb32)
    moved = (gb32[..., 6:9].astype(np.float64) - np.array([step[0], step[1], 0.0])).astype(np.float32)
    mv[..., 0:3] = np.where(obj[..., None], moved, mv[..., 0:3])
    return rgb.astype(np.float32), gb32, var.astype(np.float32), mv, clean, obj


# ------------------------------------------------------------------ the previous-position pass, replayed sample by sample
F32 = np.float32


def _m4_point(m, p):
    """ftn_math.h's m4_point in float32: column-major m, ((m0 x + m4 y) + m8 z) + m12 per row, then the product by 1 / w"""
    m, p = np.asarray(m, F32), np.asarray(p, F32)
    row = lambda r: F32(F32(F32(F32(m[r] * p[0]) + F32(m[4 + r] * p[1])) + F32(m[8 + r] * p[2])) + F32(m[12 + r] * F32(1.0)))
    e = F32(F32(1.0) / row(3))
    return np.array([F32(row(0) * e), F32(row(1) * e), F32(row(2) * e)], F32)


def _m4_normal(inv, n):
    """ftn_math.h's m4_normal with the transform's stored inverse: component r = (inv[r] x + inv[4 + r] y) + inv[8 + r] z"""
    inv, n = np.asarray(inv, F32), np.asarray(n, F32)
    return np.array([F32(F32(F32(inv[r] * n[0]) + F32(inv[4 + r] * n[1])) + F32(inv[8 + r] * n[2])) for r in range(3)], F32)


def _dot(a, b):
    return F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))


def _normalize(v):
    inv = F32(F32(1.0) / np.sqrt(_dot(v, v), dtype=F32))
    return np.array([F32(v[0] * inv), F32(v[1] * inv), F32(v[2] * inv)], F32)


def _cross(a, b):
    return np.array([F32(F32(a[1] * b[2]) - F32(a[2] * b[1])), F32(F32(a[2] * b[0]) - F32(a[0] * b[2])), F32(F32(a[0] * b[1]) - F32(a[1] * b[0]))], F32)


def _bary(b, v0, v1, v2):
    """b0 v0 + b1 v1 + b2 v2, left to right, per component"""
    return np.array([F32(F32(F32(b[0] * v0[k]) + F32(b[1] * v1[k])) + F32(b[2] * v2[k])) for k in range(3)], F32)


def previous_surface(desc, prev_desc, ins, bary, p, ns):
    """p' and ns' of the header for a hit on insertion-order primitive `ins` with barycentrics `bary`, world position p and shading normal
    ns, from the PREVIOUS scene description's vertices or transforms"""
    pr, pp = desc.prims[ins], prev_desc.prims[ins]
    assert pr.shape_kind == pp.shape_kind
    if pr.shape_kind == 1:                                                  # a sphere
        sc, sp = desc.spheres[pr.shape_index], prev_desc.spheres[pp.shape_index]
        same = all(bytes(a) == bytes(b) for a, b in ((sc.object_to_world, sp.object_to_world), (sc.world_to_object, sp.world_to_object)))
        if same:
            return np.array(p, F32), np.array(ns, F32)
        p_obj = _m4_point(sc.world_to_object.m[:], p)
        n_obj = _m4_normal(sc.world_to_object.inv[:], ns)
        return _m4_point(sp.object_to_world.m[:], p_obj), _normalize(_m4_normal(sp.object_to_world.inv[:], n_obj))
    tri = pp.shape_index
    vi = [prev_desc.tri_indices[3 * tri + k] for k in range(3)]
    P = [np.array([prev_desc.P[3 * v + k] for k in range(3)], F32) for v in vi]
    mesh = prev_desc.meshes[prev_desc.tri_mesh[tri]]
    assert not mesh.has_tangents
    pos = _bary(bary, *P)
    if mesh.has_normals:
        N = [np.array([prev_desc.N[3 * v + k] for k in range(3)], F32) for v in vi]
        return pos, _normalize(_bary(bary, *N))
    n = _normalize(_cross(P[0] - P[2], P[1] - P[2]))
    return pos, (-n if mesh.flip_normals else n)


def replay(gpu, orc, make, spp, seed, crop=(0.0, 0.0, 1.0, 1.0), tiles=None, radius=(0.5, 0.5), first_sample=0, sample_count=0, start=None, same=False):
    """The sums ftn_render_motion adds for make(be, 1) against make(be, 0) (against itself when `same`), from the oracle's camera rays,
    the current scene's ftn_intersect (primitive and barycentrics; the oracle reports none) and ftn_intersect_full (p, ns), the previous
    scene DESCRIPTION and the film rule: a pixel's own samples in increasing index into
    `start`, the samples of other pixels summed apart and added after.  The sample loop is _ao_ref.first_surfaces' with the barycentrics
    kept.  Returns dict(acc [H, W, 8], foreign [H, W], n, n_spill, rays_closest, hits, kinds: the set of (kind, moved) recorded)."""
    import ctypes as C
    import _gbuffer_ref as GR
    b, _, res = make(gpu, 1)
    _, cam, _ = make(orc, 1)
    sc = b.create_scene()
    bp, _, _ = make(gpu, 1 if same else 0)
    prev_desc, keep_prev = bp.build_desc()
    f = GR.film(orc, res, crop, radius)
    desc, (_, order) = sc.desc, sc.nodes()
    u5 = (C.c_float * 5)()
    last = first_sample + (sample_count or spp - first_sample)
    samples, rays = [], []
    for tile in GR.selected_tiles(f, tiles):
        tpb = GR.tile_pixel_bounds(f, tile)
        for py in range(tile[1], tile[3]):
            for px in range(tile[0], tile[2]):
                for s in range(first_sample, last):
                    orc.lib.orc_kat_indexed_f32(C.c_uint64(seed), C.c_int32(px), C.c_int32(py), C.c_uint32(s), u5, C.c_size_t(5))
                    u = np.array(u5[:], F32)
                    s5 = (F32(px) + u[0], F32(py) + u[1], u[2], u[3], u[4])
                    ray, _ = GR.camera_ray_differential(orc, cam, s5, spp)
                    rays.append(list(ray[0]) + list(ray[1]) + [np.inf, 0.0])
                    samples.append((px, py, s, s5, tpb))
    rays = np.array(rays, F32).reshape(-1, 8)
    full, bary, prim = np.zeros((len(rays), 24), F32), np.zeros((len(rays), 3), F32), np.full(len(rays), -1, np.int64)
    todo, n_rays = np.arange(len(rays)), 0
    spawn = (C.c_float * 8)()
    while todo.size:                       # null-material hits spawn the ray on along its direction (path.rs:77-80)
        n_rays += todo.size
        _, pr, ba, _ = sc.intersect(rays[todo], stats=False)
        fu = sc.intersect_full(rays[todo])
        full[todo], prim[todo], bary[todo] = fu, pr, ba
        again = []
        for k, i in enumerate(todo):
            if pr[k] >= 0 and desc.prims[int(order[pr[k]])].material < 0:
                orc.lib.orc_kat_spawn_ray(*((C.c_float * 3)(*fu[k, a:a + 3]) for a in (0, 3, 6)), (C.c_float * 3)(*rays[i, 3:6]), spawn)
                rays[i] = spawn[:]
                again.append(i)
        todo = np.array(again, np.int64)
    c = f.desc.crop
    acc = np.zeros((f.height, f.width, 8), F32) if start is None else np.array(start, F32)
    spill = np.zeros((f.height, f.width, 8), F32)
    foreign = np.zeros((f.height, f.width), bool)
    n_spill, hits, kinds = 0, 0, set()
    for i, (px, py, s, s5, tpb) in enumerate(samples):
        rec = None
        if prim[i] >= 0:
            ins = int(order[prim[i]])
            pp, nn = previous_surface(desc, prev_desc, ins, bary[i], full[i, 0:3], full[i, 20:23])
            kinds.add((int(desc.prims[ins].shape_kind), bool((bits32(pp) != bits32(full[i, 0:3])).any())))
            rec, hits = (pp, nn), hits + 1
        touched = GR.footprint(f, tpb, s5[0], s5[1])
        if len(touched) != 1:
            n_spill += 1
        for (x, y) in touched:
            own = (x, y) == (px, py)
            a = (acc if own else spill)[y - c[1], x - c[0]]
            if rec is not None:
                a[0:3] += rec[0] * F32(1.0)
                a[3:6] += rec[1] * F32(1.0)
                a[6] += F32(1.0)
            a[7] += F32(1.0)
            if not own:
                foreign[y - c[1], x - c[0]] = True
    acc += spill
    return dict(acc=acc, foreign=foreign, n=len(samples), n_spill=n_spill, rays_closest=n_rays, hits=hits, kinds=kinds, keep=(b, cam, bp, keep_prev))


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_replayed(raw, ref, what="", rtol=2e-6, atol=1e-6):
    """the two weights equal on every pixel; position and normal sums bit-equal where no sample of another pixel landed, and within the
    tolerance of the film's reordered spill sums (tests/test_gbuffer.py's) where one did"""
    want = ref["acc"]
    assert np.array_equal(bits32(raw[..., 6:8]), bits32(want[..., 6:8])), "%s: weights differ at %d pixels" % (what, int((raw[..., 6:8] != want[..., 6:8]).any(-1).sum()))
    diff = (bits32(raw[..., :6]) != bits32(want[..., :6])).any(-1)
    bad = diff & ~ref["foreign"]
    assert not bad.any(), "%s: sums differ at %d pixels outside spill pixels, first %r: %r against %r" % (
        what, int(bad.sum()), tuple(np.argwhere(bad)[0]), raw[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])
    assert np.allclose(raw, want, rtol=rtol, atol=atol), "%s: beyond the spill tolerance" % what
