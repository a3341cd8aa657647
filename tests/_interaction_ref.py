"""A binary64 restatement of the reference's surface interactions, ray differentials and camera rays, written from the Rust (cited by file and
line under src/) and from neither C++ copy: shapes/triangle.rs:176-393, shapes/sphere.rs:83-200, interaction.rs:22-30 and :124-173,
geometry/mod.rs (coordinate_system :53-62, faceforward :64-70, offset_ray_origin :72-85, scale_differentials :125-133), math.rs:56-72,
camera/mod.rs:145-205, geometry/transform.rs (rays :307-338, hits and interactions :340-385, normals :133-139 as written),
integrator/mod.rs:58-84 and :119-163.  The hit tests, the transforms and offset_ray_origin are the ones tests/_light_ref.py restates.

It reads what a SceneBuilder and a camera description hold and the rows of the hooks (tests/_interaction_common.py); everything is evaluated
in binary64 on the binary32 inputs, and a row where binary32 rounding may send the reference down another branch is flagged `fragile`."""
import numpy as np

import _interaction_common as K
import _light_ref as R
from _light_ref import EPS, cross, dot, gamma, normalize

from _interaction_common import MAX_FRAGILE_SHARE, MEASURED, MEASURED_CAMERA, MEASURED_FRAGILE_SHARE, ON_SURFACE, TOL_CAMERA, TOLERANCE

UNIT = ["n", "wo", "ns", "rxd", "ryd", "bary", "uv"]                  # floor 1e-3
POSITIONS = ["p", "spawn_o", "rxo", "ryo", "t"]                       # floor 1e-3 x the primitive's extent
VECTORS = ["p_err", "s_dpdu", "dpdu", "dpdv", "dndu", "dndv", "dpdx", "dpdy", "duvdx", "duvdy"]      # floor 1e-3 x the row's largest component of the vector


def coordinate_system(v1):                            # geometry/mod.rs:53-62 -> (v2, v3)
    a = normalize(np.stack([-v1[:, 2], np.zeros(len(v1)), v1[:, 0]], axis=1))
    b = normalize(np.stack([np.zeros(len(v1)), v1[:, 2], -v1[:, 1]], axis=1))
    v2 = np.where((np.abs(v1[:, 0]) > np.abs(v1[:, 1]))[:, None], a, b)
    return v2, cross(v1, v2)


def triangle(g, o, d, t_max):
    """shapes/triangle.rs:176-393 -> the interaction's fields in binary64, `hit`, `fragile`"""
    m = len(o)
    h = g.hit_test(o, d, t_max)                       # :176-268, :277-288
    b, fragile = h["bary"], h["fragile"].copy()
    p0, p1, p2 = g.p
    uv = g.uv                                         # :131-143 (defaults without uvs)
    duv02, duv12, dp02, dp12 = uv[0] - uv[2], uv[1] - uv[2], p0 - p2, p1 - p2
    det = duv02[0] * duv12[1] - duv02[1] * duv12[0]   # :277
    assert abs(abs(det) - 1.0e-8) > 1.0e-3 * 1.0e-8, "the uv determinant is within rounding of 1e-8"
    degenerate = abs(det) < 1.0e-8
    if degenerate:                                    # :280-288
        ng = cross(p2 - p0, p1 - p0)
        dpdu, dpdv = coordinate_system(normalize(ng)[None])
        dpdu, dpdv = dpdu[0], dpdv[0]
    else:                                             # :290-293
        dpdu = (duv12[1] * dp02 - duv02[1] * dp12) / det
        dpdv = (-duv12[0] * dp02 + duv02[0] * dp12) / det
    with np.errstate(all="ignore"):
        p_err = gamma(7) * (np.abs(b[:, 0:1] * p0) + np.abs(b[:, 1:2] * p1) + np.abs(b[:, 2:3] * p2))      # :296-299
        p = b @ g.p                                   # :302
        uv_hit = b @ uv                               # :303
        n = normalize(cross(dp02, dp12))              # :314
        if g.flip:                                    # :326-329
            n = -n
        n = np.broadcast_to(n, (m, 3)).copy()
        ns, s_dpdu = n.copy(), np.broadcast_to(dpdu, (m, 3)).copy()
        dndu, dndv = np.zeros((m, 3)), np.zeros((m, 3))
        if g.n is not None or g.s is not None:        # :331-391
            if g.n is not None:
                ns = normalize(b @ g.n)
            ss = normalize(b @ g.s) if g.s is not None else np.broadcast_to(normalize(dpdu), (m, 3))
            ts = cross(ns, ss)
            l2 = dot(ts, ts)
            fragile |= (l2 > 0.0) & (l2 <= 1.0e-9)    # len2(ts) within rounding of 0
            v2, v3 = coordinate_system(ns)            # (ts, ss) = (v2, v3), :349
            s_dpdu = np.where((l2 > 0.0)[:, None], cross(normalize(ts), ns), v3)
            if g.n is not None:
                dn1, dn2 = g.n[0] - g.n[2], g.n[1] - g.n[2]
                if degenerate:                        # :356-365
                    dn = cross(g.n[2] - g.n[0], g.n[1] - g.n[0])
                    if dot(dn, dn) != 0.0:
                        a, c = coordinate_system(dn[None])
                        dndu, dndv = np.broadcast_to(a[0], (m, 3)).copy(), np.broadcast_to(c[0], (m, 3)).copy()
                else:                                 # :366-369: `inv_det` is the BARYCENTRIC one, the uv one went out of scope at :294
                    dndu = (duv12[1] * dn1 - duv02[1] * dn2)[None] * h["inv_det"][:, None]
                    dndv = (-duv12[0] * dn1 + duv02[0] * dn2)[None] * h["inv_det"][:, None]
            dd = dot(n, ns)                           # :389
            fragile |= np.abs(dd) <= 1.0e-5
            n = np.where((dd < 0.0)[:, None], -n, n)
    z = lambda v: np.broadcast_to(v, (m, 3)).copy()
    return dict(hit=~h["miss"], fragile=fragile, t=h["t"], bary=b, p=p, p_err=p_err, n=n, wo=-d, ns=ns, s_dpdu=s_dpdu, uv=uv_hit, dpdu=z(dpdu), dpdv=z(dpdv),
                dndu=dndu, dndv=dndv, root=np.zeros(m, int))


def sphere(g, o, d, t_max):
    """shapes/sphere.rs:83-200 and SurfaceInteraction::transform (transform.rs:369-385)"""
    m = len(o)
    hit, p_w, n_w, fragile, which, p, t, (oo, dd) = g.intersect(o, d, t_max)
    with np.errstate(all="ignore"):
        # what the object-space origin is off by (transform.rs:230-243) against the limb, the roots and t_max: a sphere that is small beside its
        # distance from the world's origin loses that share of its radius to the translation
        W = g.w2o
        err = R.norm(gamma(3) * (np.abs(o) @ np.abs(W[:3, :3]).T + np.abs(W[:3, 3])))
        ld = R.norm(dd)
        t0, t1 = g.roots(o, d)
        limb = np.abs(R.norm(cross(oo, dd)) / ld - g.r) <= 16.0 * err
        near = np.minimum.reduce([np.abs(t0), np.abs(t1), np.abs(t0 - t_max), np.abs(t1 - t_max)]) <= 16.0 * err / ld
        fragile = fragile | limb | (near & np.isfinite(t0))
        phi = np.arctan2(p[:, 1], p[:, 0]); phi = np.where(phi < 0.0, phi + 2.0 * np.pi, phi)
        u = phi / g.phi_max                           # :146
        theta = np.arccos(np.clip(p[:, 2] / g.r, -1.0, 1.0))
        dth = g.theta_max - g.theta_min
        v = (theta - g.theta_min) / dth
        zr = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2)
        cphi, sphi = p[:, 0] / zr, p[:, 1] / zr
        zero = np.zeros(m)
        dpdu = np.stack([-g.phi_max * p[:, 1], g.phi_max * p[:, 0], zero], axis=1)
        dpdv = dth * np.stack([p[:, 2] * cphi, p[:, 2] * sphi, -g.r * np.sin(theta)], axis=1)
        d2uu = (-g.phi_max * g.phi_max) * np.stack([p[:, 0], p[:, 1], zero], axis=1)        # :159-162
        d2uv = (dth * p[:, 2] * g.phi_max)[:, None] * np.stack([-sphi, cphi, zero], axis=1)
        d2vv = -dth * dth * p
        E, F, G = dot(dpdu, dpdu), dot(dpdu, dpdv), dot(dpdv, dpdv)
        N = normalize(cross(dpdu, dpdv))
        e, f, gg = dot(N, d2uu), dot(N, d2uv), dot(N, d2vv)
        inv = 1.0 / (E * G - F * F)
        dndu = ((f * F - e * G) * inv)[:, None] * dpdu + ((e * F - f * E) * inv)[:, None] * dpdv       # :176
        dndv = ((gg * F - f * G) * inv)[:, None] * dpdu + ((f * F - gg * E) * inv)[:, None] * dpdv     # :178
        err = gamma(5) * np.abs(p)                    # :180
        M = g.o2w                                     # transform.rs:245-264
        p_err = (gamma(3) + 1.0) * (err @ np.abs(M[:3, :3]).T) + gamma(3) * (np.abs(p) @ np.abs(M[:3, :3]).T + np.abs(M[:3, 3]))
        wo = normalize(R.tf_vector(M, -dd))
    return dict(hit=hit, fragile=fragile, t=t, bary=np.zeros((m, 3)), p=p_w, p_err=p_err, n=n_w, wo=wo, ns=n_w, s_dpdu=R.tf_vector(M, dpdu), uv=np.stack([u, v], axis=1),
                dpdu=R.tf_vector(M, dpdu), dpdv=R.tf_vector(M, dpdv), dndu=R.tf_normal(g.o2w_inv, dndu), dndv=R.tf_normal(g.o2w_inv, dndv), root=which)


def solve_2x2(a00, a01, a10, a11, b0, b1):            # math.rs:56-72, A = from_cols((a00, a01), (a10, a11)) -> x0, x1, solved, fragile
    with np.errstate(all="ignore"):
        det = a00 * a11 - a10 * a01
        x0, x1 = (a11 * b0 - a10 * b1) / det, (a00 * b1 - a01 * b0) / det
        ok = ~(np.abs(det) < 1.0e-10) & ~np.isnan(x0) & ~np.isnan(x1)
        fragile = np.abs(np.abs(det) - 1.0e-10) <= 1.0e-3 * 1.0e-10 + 64.0 * EPS * (np.abs(a00 * a11) + np.abs(a10 * a01))
    return x0, x1, ok, fragile


def tex_differentials(s, has, rxo, ryo, rxd, ryd):    # interaction.rs:124-173
    n, p = s["n"], s["p"]
    m = len(p)
    with np.errstate(all="ignore"):
        dd = dot(n, p)
        px = rxo + (-(dot(n, rxo) - dd) / dot(n, rxd))[:, None] * rxd
        py = ryo + (-(dot(n, ryo) - dd) / dot(n, ryd))[:, None] * ryd
        dpdx, dpdy = px - p, py - p
        an = np.abs(n)
        first = (an[:, 0] > an[:, 1]) & (an[:, 0] > an[:, 2])
        second = ~first & (an[:, 1] > an[:, 2])
        srt = np.sort(an, axis=1)
        tie = (srt[:, 2] - srt[:, 1]) <= 1.0e-5       # the largest |n| component is not clearly the largest
        d0, d1 = np.where(first, 1, 0), np.where(first | second, 2, 1)
        r = np.arange(m)
        A = s["dpdu"][r, d0], s["dpdu"][r, d1], s["dpdv"][r, d0], s["dpdv"][r, d1]
        dudx, dvdx, okx, fx = solve_2x2(*A, dpdx[r, d0], dpdx[r, d1])
        dudy, dvdy, oky, fy = solve_2x2(*A, dpdy[r, d0], dpdy[r, d1])
        # a grazing auxiliary ray: the quotient's error grows with 1 / (n . rxd)
        graze = (np.abs(dot(n, rxd)) <= 1.0e-3 * R.norm(rxd)) | (np.abs(dot(n, ryd)) <= 1.0e-3 * R.norm(ryd))
    ok = (has != 0.0) & okx & oky
    z = lambda v: np.where(ok[:, None] if v.ndim == 2 else ok, v, 0.0)
    return dict(dpdx=z(dpdx), dpdy=z(dpdy), dudx=z(dudx), dvdx=z(dvdx), dudy=z(dudy), dvdy=z(dvdy), solved=ok), (has != 0.0) & (tie | fx | fy | graze)


def specular(s, td, has, rxd, ryd, wi, eta, reflect):
    """integrator/mod.rs:58-84 (reflect), :119-163 (transmit), as written -> rxo ryo rxd ryd, fragile"""
    p, wo, ns0 = s["p"], s["wo"], s["ns"]
    with np.errstate(all="ignore"):
        dndx = s["dndu"] * td["dudx"][:, None] + s["dndv"] * td["dvdx"][:, None]
        dndy = s["dndu"] * td["dudy"][:, None] + s["dndv"] * td["dvdy"][:, None]
        dwx, dwy = -rxd - wo, -ryd - wo
        # reflect :66-75
        rx_r = (wi - dwx) + (2.0 * dot(wo, ns0))[:, None] * dndx + (dot(dwx, ns0) + dot(wo, dndx))[:, None] * ns0
        ry_r = (wi - dwy) + (2.0 * dot(wo, ns0))[:, None] * dndy + (dot(dwy, ns0) + dot(wo, dndy))[:, None] * ns0
        # transmit :124-156
        leaving = dot(wo, ns0) < 0.0
        e = np.where(leaving, eta, 1.0 / eta)
        sn = np.where(leaving[:, None], -ns0, ns0)
        fx, fy = np.where(leaving[:, None], -dndx, dndx), np.where(leaving[:, None], -dndy, dndy)
        dDNx, dDNy = dot(dwx, ns0) + dot(wo, fx), dot(dwy, ns0) + dot(wo, fy)          # :141-142: the unflipped shading normal
        mu = e * dot(wo, sn) - np.abs(dot(wi, sn))
        k = e - (e * e * dot(wo, sn)) / dot(wi, sn)
        rx_t = wi - e[:, None] * dwx + (mu[:, None] * fx + (k * dDNx)[:, None] * sn)
        ry_t = wi - e[:, None] * dwy + (mu[:, None] * fy + (k * dDNy)[:, None] * sn)
        refl = (reflect != 0.0)[:, None]
        on = (has != 0.0)[:, None]
        out = dict(rxo=np.where(on, p + td["dpdx"], 0.0), ryo=np.where(on, p + td["dpdy"], 0.0), rxd=np.where(on, np.where(refl, rx_r, rx_t), 0.0), ryd=np.where(on, np.where(refl, ry_r, ry_t), 0.0))
        fragile = (has != 0.0) & (reflect == 0.0) & ((np.abs(dot(wo, ns0)) <= 1.0e-5) | (np.abs(dot(wi, sn)) <= 1.0e-3 * R.norm(wi)))
    return out, fragile


def evaluate(geo, rows):
    r = np.asarray(rows, np.float64)
    k = K.prim_of(np.ascontiguousarray(rows))
    m = len(r)
    out = {}
    for i, g in enumerate(geo):
        sel = np.flatnonzero(k == i)
        if not len(sel):
            continue
        part = (triangle if g.kind == "tri" else sphere)(g, r[sel, 0:3], r[sel, 3:6], r[sel, 6])
        for key, val in part.items():
            if key not in out:
                out[key] = np.zeros((m,) + val.shape[1:], val.dtype)
            out[key][sel] = val
    has, wi = r[:, 9], r[:, 22:25]
    td, f_td = tex_differentials(out, has, r[:, 10:13], r[:, 13:16], r[:, 16:19], r[:, 19:22])
    sp, f_sp = specular(out, td, has, r[:, 16:19], r[:, 19:22], wi, r[:, 25], r[:, 26])
    out.update(td); out.update(sp)
    out["spawn_o"] = R.offset_ray_origin(out["p"], out["p_err"], out["n"], wi)          # interaction.rs:22-30, geometry/mod.rs:72-85
    with np.errstate(all="ignore"):
        out["fragile"] = out["fragile"] | (out["hit"] & (f_td | f_sp | (np.abs(dot(wi, out["n"])) <= 1.0e-6 * R.norm(wi))))
    out["duvdx"], out["duvdy"] = np.stack([out["dudx"], out["dvdx"]], axis=1), np.stack([out["dudy"], out["dvdy"]], axis=1)
    out["time"] = r[:, 7]
    return out


def compare_with_restatement(hook, rows, report=None):
    """-> (99.9th percentile, maximum of the metric over the compared values, share of rows left out).  Asserts the discrete outcomes on the rows
    that are compared: hit or miss, which root, material and light, zero or nonzero differentials"""
    want = evaluate(hook.targets, rows)
    got = hook(rows)
    got["duvdx"], got["duvdy"] = np.stack([got["dudx"], got["dvdx"]], axis=1), np.stack([got["dudy"], got["dvdy"]], axis=1)
    keep = ~want["fragile"]
    assert np.array_equal(got["hit"][keep], want["hit"][keep]), (hook.name, "hit or miss", int((got["hit"] != want["hit"])[keep].sum()))
    m = keep & want["hit"]
    k = K.prim_of(rows)
    extent = np.array([g.radius for g in hook.targets])[k]
    assert np.all(got["mat"][m] == 1), "the matte material the scene sets"
    emitting = hook.name in K.TRIANGLES and hook.name != "tri_uv"
    lights = [set(got["light"][m & (k == i)].tolist()) for i in range(len(hook.targets))]
    assert all(len(s) <= 1 for s in lights) and sorted(x for s in lights for x in s) == (list(range(len(lights))) if emitting else [-1] * len(lights)), (hook.name, lights)
    assert np.array_equal(got["time"][m], want["time"][m])
    r64 = np.asarray(rows, np.float64)
    for g_i, g in enumerate(hook.targets):            # which root: the returned t is nearer one of the two binary64 roots; that index against the restated one
        if g.kind == "sph":
            mm = m & (k == g_i)
            t0, t1 = g.roots(r64[mm, 0:3], r64[mm, 3:6])
            got_root = (np.abs(got["t"][mm] - t1) < np.abs(got["t"][mm] - t0)).astype(int)
            assert np.array_equal(got_root, want["root"][mm]), (hook.name, "another root", int((got_root != want["root"][mm]).sum()))
    nz = lambda o: (np.abs(o["dudx"]) + np.abs(o["dvdx"]) + np.abs(o["dudy"]) + np.abs(o["dvdy"]) + np.abs(o["dpdx"]).sum(axis=1)) != 0.0
    assert np.array_equal(nz(got)[m], want["solved"][m] & nz(want)[m]), (hook.name, "zero or nonzero differentials")
    errs = []
    with np.errstate(all="ignore"):
        for c in UNIT:
            errs.append(K_rel(got[c][m], want[c][m], 1.0e-3))
        for c in POSITIONS:
            errs.append(K_rel(got[c][m], want[c][m], (1.0e-3 * extent[m])[:, None] if got[c].ndim == 2 else 1.0e-3 * extent[m]))
        for c in VECTORS:
            errs.append(K_rel(got[c][m], want[c][m], 1.0e-3 * np.abs(want[c][m]).max(axis=1, keepdims=True)))
    if report is not None:
        for c, x in zip(UNIT + POSITIONS + VECTORS, errs):
            report[c] = (float(np.percentile(x, 99.9)), float(x.max()))
    e = np.concatenate([x.ravel() for x in errs])
    return float(np.percentile(e, 99.9)), float(e.max()), float(np.mean(want["fragile"]))


def K_rel(got, want, floor):
    e = np.abs(got - want) / np.maximum(np.abs(want), floor)
    e = np.where((np.isnan(got) & np.isnan(want)) | (got == want), 0.0, e)
    return np.where(np.isnan(e), np.inf, e)


# ---------------------------------------------------------------- camera/mod.rs:145-205
def concentric_sample_disk(u):                        # sampling.rs:5-19
    uo = 2.0 * u - 1.0
    with np.errstate(all="ignore"):
        wide = np.abs(uo[:, 0]) > np.abs(uo[:, 1])
        theta = np.where(wide, np.pi / 4.0 * (uo[:, 1] / uo[:, 0]), np.pi / 2.0 - np.pi / 4.0 * (uo[:, 0] / uo[:, 1]))
        rr = np.where(wide, uo[:, 0], uo[:, 1])
        out = rr[:, None] * np.stack([np.cos(theta), np.sin(theta)], axis=1)
    return np.where(((uo[:, 0] == 0.0) & (uo[:, 1] == 0.0))[:, None], 0.0, out)


def tf_point_h(m, p):
    """cgmath's Matrix4::transform_point: the homogeneous divide (raster_to_camera is projective)"""
    q = p @ m[:3, :3].T + m[:3, 3]
    w = p @ m[3, :3] + m[3, 3]
    return q / w[:, None]


def camera(desc, spp, rows):
    r = np.asarray(rows, np.float64)
    m = len(r)
    c2w, _ = R.mat(desc.camera_to_world)
    r2c, _ = R.mat(desc.raster_to_camera)
    dxc, dyc = np.array(desc.dx_camera[:], np.float64), np.array(desc.dy_camera[:], np.float64)
    lens_radius, focal = float(desc.lens_radius), float(desc.focal_dist)
    pc = tf_point_h(r2c, np.stack([r[:, 0], r[:, 1], np.zeros(m)], axis=1))              # :146-147
    time = (1.0 - r[:, 4]) * float(desc.shutter_open) + r[:, 4] * float(desc.shutter_close)      # :148, math.rs lerp
    o = np.zeros((m, 3))
    d = normalize(pc)
    fragile = np.zeros(m, bool)
    if lens_radius > 0.0:                             # :154-182
        pl = lens_radius * concentric_sample_disk(r[:, 2:4])
        lo = np.stack([pl[:, 0], pl[:, 1], np.zeros(m)], axis=1)
        fragile |= np.abs(d[:, 2]) <= 1.0e-6
        pf = d * (focal / d[:, 2])[:, None]
        o, d = lo, normalize(pf - lo)
        dx = normalize(pc + dxc)
        rxo, rxd = lo, normalize(dx * (focal / dx[:, 2])[:, None] - lo)
        dy = normalize(pc + dxc)                      # :173: dx_camera
        ryo, ryd = lo, normalize(dy * (focal / dy[:, 2])[:, None] - lo)
    else:                                             # :183-197
        rxo, ryo, rxd, ryd = o, o, normalize(pc + dxc), normalize(pc + dyc)
    # Ray::transform, transform.rs:307-322
    ow, dw = R.tf_point(c2w, o), R.tf_vector(c2w, d)
    o_err = gamma(3) * (np.abs(o) @ np.abs(c2w[:3, :3]).T + np.abs(c2w[:3, 3]))
    dt = dot(np.abs(dw), o_err) / dot(dw, dw)
    ow = ow + dw * dt[:, None]
    rxo, ryo, rxd, ryd = R.tf_point(c2w, rxo), R.tf_point(c2w, ryo), R.tf_vector(c2w, rxd), R.tf_vector(c2w, ryd)
    s = 1.0 / np.sqrt(np.float32(spp))                # integrator/mod.rs:254, geometry/mod.rs:125-133
    return dict(o=ow, d=dw, t_max=np.full(m, np.inf), time=time, rxo=ow + (rxo - ow) * s, ryo=ow + (ryo - ow) * s, rxd=dw + (rxd - dw) * s, ryd=dw + (ryd - dw) * s, fragile=fragile)


def compare_camera(be, name, spp, rows):
    cam = K.cameras(be)[name][0]
    got = K.camera_raw(be, cam, spp, rows).astype(np.float64)
    want = camera(cam.desc, spp, rows)
    keep = ~want["fragile"]
    size = np.abs(want["o"]).max() + 1.0
    errs = [K_rel(got[keep][:, K.CAM[c]], want[c][keep], 1.0e-3 * (size if c in ("o", "rxo", "ryo") else 1.0)) for c in ("o", "d", "time", "rxo", "ryo", "rxd", "ryd")]
    assert np.all(got[:, 6] == np.inf)
    return float(max(e.max() for e in errs)), float(np.mean(want["fragile"]))
