"""A binary64 restatement of the reference's integrators, written from the Rust (cited by file and line under src/) and from none of the three
C++ copies (oracle/orc_render.hpp, the megakernel and the wavefront state machine of fountain_amd/csrc): integrator/mod.rs:229-395
(render_tile's per-sample body, uniform_sample_one_light, estimate_direct) and :39-178 (specular_reflect / specular_transmit), integrator/path.rs:25-95,
integrator/direct_lighting.rs:50-106, integrator/whitted.rs:20-71, scene/mod.rs:32-64, interaction.rs:22-58 and :111-121 and :175-180,
light/mod.rs:82-84, light/diffuse.rs:44-50, sampling.rs:53-57, sampler/mod.rs:43-51.

It strings together the restatements that exist already and re-derives none of them: _bsdf_ref (Bsdf.f / pdf / sample_f and the materials' lobes),
_light_ref (the lights, offset_ray_origin, the hit tests), _interaction_ref (interactions, texture and specular differentials, camera rays),
_texture_ref (textured material parameters).  It reads what a SceneBuilder and a camera description hold.  Scene::intersect and
Scene::intersect_test go over every primitive (no BVH).  One thing comes from a library: the order of the area lights in Scene::lights when more than
one primitive emits, which is the BVH's primitive order (scene/mod.rs:38-42); the caller hands it in as `area_order`.

The indexed sampler is this project's ("Sampler"): the reference's generator and draw order, re-seeded per (pixel, sample) from
indexed_key.  It is restated in exact integer arithmetic.

Everything is vectorised over camera samples, bounce by bounce.  A sample on which binary32 rounding may take another branch than binary64 is
flagged `fragile`, by the predicates of the imported restatements and those added here (the roulette's u - q, u * n_lights against an integer, the
emission's cosine, a tie between the two nearest hits, values in binary32's underflow range)."""
import numpy as np

import _bsdf_ref as B
import _interaction_common as IK
import _interaction_ref as IR
import _light_ref as R
import _texture_ref as T
from _light_ref import dot, gamma
from fountain_amd import _abi as A

NONSPEC = B.ALL & ~B.SPECULAR
TOL = 1.0e-4                                          # the branch margin of _bsdf_ref.evaluate's default
TINY = 1.0e-30                                        # a nonzero value below this may be 0 in binary32
SHADOW_T_MAX = float(np.float32(1.0) - np.float32(0.0001))          # interaction.rs:10, :55
U64 = np.uint64
MASK64 = (1 << 64) - 1


def black(x):                                         # spectrum/mod.rs:76-78
    return np.all(x == 0.0, axis=-1)


def power_heuristic(f_pdf, g_pdf):                    # sampling.rs:53-57 with nf = ng = 1
    with np.errstate(all="ignore"):
        return (f_pdf * f_pdf) / (f_pdf * f_pdf + g_pdf * g_pdf)


def close(margins, n):
    out = np.zeros(n, bool)
    for m in margins:
        out |= ~(m >= TOL)
    return out


def tiny(x):
    a = np.abs(x)
    return np.any((a > 0.0) & (a < TINY), axis=-1) if a.ndim > 1 else (a > 0.0) & (a < TINY)


# ---------------------------------------------------------------- the indexed sampler
def indexed_key(seed, px, py, sample):
    """(seed * golden) ^ (py << 40) ^ (px << 20) ^ sample, in Python integers"""
    return ((seed * 0x9E3779B97F4A7C15) & MASK64) ^ ((py & 0xFFFFFFFF) << 40) ^ ((px & 0xFFFFFFFF) << 20) ^ sample


def splitmix64(x):
    """one step of SplitMix64 (rand_xoshiro 0.2.0's seed_from_u64) on a Python integer -> (state, output)"""
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return x, z ^ (z >> 31)


def scalar_floats(seed, px, py, sample, n):
    """the first n floats of one (pixel, sample), in Python integers: the check of Rng"""
    x = indexed_key(seed, px, py, sample)
    s = []
    for _ in range(4):
        x, z = splitmix64(x)
        s.append(z)
    out = []
    for _ in range(n):                                # Xoshiro256+: result = s0 + s3 before the state moves
        result = (s[0] + s[3]) & MASK64
        t = (s[1] << 17) & MASK64
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]
        s[2] ^= t
        s[3] = ((s[3] << 45) | (s[3] >> 19)) & MASK64
        out.append(((result >> 32) >> 8) * 2.0 ** -24)                # next_u32 = the upper half; rand 0.6.5 Standard: 24 bits in [0, 1)
    return out


class Rng:
    """one Xoshiro256+ state per camera sample, uint64 arithmetic (numpy wraps silently on arrays)"""

    def __init__(self, seed, px, py, sample):
        g = U64(0x9E3779B97F4A7C15)
        with np.errstate(over="ignore"):
            x = np.full(len(px), (seed * 0x9E3779B97F4A7C15) & MASK64, U64)
            x = x ^ (py.astype(np.int64).astype(U64) & U64(0xFFFFFFFF)) << U64(40) ^ (px.astype(np.int64).astype(U64) & U64(0xFFFFFFFF)) << U64(20) ^ sample.astype(U64)
            s = []
            for _ in range(4):
                x = x + g
                z = x
                z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
                z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
                s.append(z ^ (z >> U64(31)))
        self.s = np.stack(s, axis=1)
        self.draws = np.zeros(len(px), np.int64)

    def f(self, idx):
        s = self.s[idx]
        with np.errstate(over="ignore"):
            result = s[:, 0] + s[:, 3]
            t = s[:, 1] << U64(17)
            s[:, 2] ^= s[:, 0]; s[:, 3] ^= s[:, 1]; s[:, 1] ^= s[:, 2]; s[:, 0] ^= s[:, 3]
            s[:, 2] ^= t
            s[:, 3] = (s[:, 3] << U64(45)) | (s[:, 3] >> U64(19))
        self.s[idx] = s
        self.draws[idx] += 1
        return (result >> U64(40)).astype(np.float64) * 2.0 ** -24

    def f2(self, idx):                                # get_2d: x first
        a = self.f(idx)
        return np.stack([a, self.f(idx)], axis=1)


# ---------------------------------------------------------------- the scene
KIND = {A.FTN_MAT_MATTE: "matte", A.FTN_MAT_MIRROR: "mirror", A.FTN_MAT_PLASTIC: "plastic", A.FTN_MAT_METAL: "metal", A.FTN_MAT_GLASS: "glass"}


def material_keywords(m):
    """an ftn_material as the SceneBuilder.material keywords it was made from (api.py: SceneBuilder.material)"""
    a, b = [float(x) for x in m.a], [float(x) for x in m.b]
    remap = bool(m.remap_roughness)
    if m.type == A.FTN_MAT_MATTE:
        return dict(Kd=a, sigma=float(m.s0))
    if m.type == A.FTN_MAT_MIRROR:
        return dict(Kr=a)
    if m.type == A.FTN_MAT_PLASTIC:
        return dict(Kd=a, Ks=b, roughness=float(m.s1), remaproughness=remap)
    if m.type == A.FTN_MAT_METAL:
        return dict(eta=a, k=b, uroughness=float(m.s1), vroughness=float(m.s2), remaproughness=remap)
    return dict(Kr=a, Kt=b, eta=float(m.s0), uroughness=float(m.s1), vroughness=float(m.s2), remaproughness=remap)


def sub_bsdf(bsdf, sel):
    """the rows `sel` of a Bsdf"""
    lobes = []
    for l in bsdf.lobes:
        if l.r.ndim == 2:
            l2 = B.Lobe(l.kind, l.r[sel], l.fresnel, l.a, l.b, l.ax, l.ay, l.eta_a, l.eta_b)
        else:
            l2 = l
        lobes.append(l2)
    out = B.Bsdf.__new__(B.Bsdf)
    out.lobes, out.ng, out.ns, out.ss, out.ts = lobes, bsdf.ng[sel], bsdf.ns[sel], bsdf.ss[sel], bsdf.ts[sel]
    return out


FIELDS = ["t", "p", "p_err", "n", "wo", "ns", "s_dpdu", "uv", "dpdu", "dpdv", "dndu", "dndv"]


def rows_of(S, sel):
    return {k: v[sel] for k, v in S.items()}


class SceneRef:
    def __init__(self, builder, area_order=None):
        b = builder
        self.geo = IK.geometry(b)
        self.mat, self.area = [], []
        for p in b.prims:
            if p[0] == "trirange":
                self.mat += [p[3]] * p[2]; self.area += [p[4]] * p[2]
            else:
                self.mat.append(p[2]); self.area.append(p[3])
        self.mat, self.area = np.array(self.mat, np.int64), np.array(self.area, np.int64)
        self.materials = b.materials
        self.tex = T.Ref(b)
        self.textured = self.tex.mtex is not None
        _, radius = R.world_bound(b)                  # Light::preprocess(&primitives), scene/mod.rs:34-36
        self.lights = []
        for l in b.lights:                            # scene/mod.rs:32-49: the explicit lights, then the emitting primitives
            rgb, v = np.array(l.rgb[:], np.float64), np.array(l.v[:], np.float64)
            if l.type == A.FTN_LIGHT_POINT:
                self.lights.append(dict(kind="point", I=rgb, p=v))
            elif l.type == A.FTN_LIGHT_DISTANT:
                self.lights.append(dict(kind="distant", L=rgb, d=v, radius=radius))
            else:
                m, inv = R.mat(l.light_to_world)
                self.lights.append(dict(kind="infinite", env=R.EnvLight(b.envmaps[l.envmap], m, inv), radius=radius))
        emitting = [int(i) for i in np.flatnonzero(self.area >= 0)]
        if area_order is None:
            assert len(emitting) <= 1, "more than one emitting primitive: Scene::lights follows the BVH's order, hand it in"
            area_order = emitting
        assert sorted(int(i) for i in area_order) == emitting
        self.emit = np.zeros((len(self.geo), 3))
        self.light_of_prim = np.full(len(self.geo), -1, np.int64)
        for i in area_order:
            self.light_of_prim[i] = len(self.lights)
            self.emit[i] = np.array(b.area_emit[self.area[i]], np.float64)
            self.lights.append(dict(kind="area", L=self.emit[i], shape=self.geo[i]))

    # ---- Scene::intersect / intersect_test (scene/mod.rs:51-57) over every primitive
    def sphere_fragile(self, g, o, d, t_max, with_reach=False):
        """what the sphere's error intervals (sphere.rs:95-110, :126) may decide otherwise than binary64: a ray at the limb, a positive root within
        the origin's transformation error of 0 (the intervals are conservative: a root that is <= 0 stays so), a root just below t_max, a hit at a
        clip of a partial sphere.  with_reach: -> (fragile, reach), reach = how far a root may move"""
        with np.errstate(all="ignore"):
            W = g.w2o
            oo, dd = R.tf_point(W, o), R.tf_vector(W, d)
            err = R.norm(gamma(3) * (np.abs(o) @ np.abs(W[:3, :3]).T + np.abs(W[:3, 3])))
            ld = R.norm(dd)
            axis = R.norm(np.cross(oo, dd)) / ld
            limb = np.abs(axis - g.r) <= 16.0 * err + 1.0e-6 * g.r
            # a root moves by the origin's error over the sine of the angle at which the ray meets the surface
            reach = (16.0 * err + 1.0e-6 * g.r) / (ld * np.sqrt(np.maximum(g.r * g.r - axis * axis, 0.0)) / g.r)
            t0, t1 = g.roots(o, d)
            frag = limb.copy()
            partial = g.z_min > -g.r or g.z_max < g.r or g.phi_max < 2.0 * np.pi
            for t in (t0, t1):
                frag |= (axis < g.r) & (((t > 0.0) & (t <= reach)) | ((t <= t_max) & (t >= t_max - reach)))
                if partial:
                    p, phi = g.at(oo, dd, t)
                    frag |= (axis < g.r) & (t > 0.0) & (t <= t_max) & g.near_a_clip(p, phi)
            # the reference's quirk: next_float_down(0.0) is NaN (err_float.rs:22-30: -0.0 >= 0.0 holds), so a product that is exactly 0 -- an
            # object-space direction or origin component that is 0 -- leaves NaN in the intervals of a, b or c, f32::min / max then drop it,
            # and the tests of sphere.rs:99-110 go by what is left: hit or miss is not what binary64 says
            o_mag = np.abs(o) @ np.abs(W[:3, :3]).T + np.abs(W[:3, 3])
            o_err = gamma(3) * o_mag
            shifted = oo + dd * (dot(np.abs(dd), o_err) / (ld * ld))[:, None]               # transform.rs:291-296
            zero = (np.abs(dd) <= 4.0 * R.EPS * (np.abs(d) @ np.abs(W[:3, :3]).T) + 1.0e-18).any(axis=1) | (np.abs(shifted) <= 4.0 * R.EPS * o_mag + 1.0e-18).any(axis=1)
            frag |= (axis < g.r) & zero
        return (frag, reach) if with_reach else frag

    def intersect(self, o, d, t_max=None):
        """-> the nearest hit's interaction (FIELDS), `hit`, `prim` (the builder's index), `fragile`; t_max per ray, infinity by default"""
        m = len(o)
        t_max = np.full(m, np.inf) if t_max is None else np.asarray(t_max, np.float64)
        parts, ts, raws, frs = [], [], [], []
        for g in self.geo:
            if g.kind == "tri":
                s = IR.triangle(g, o, d, t_max)
                f = s["fragile"]
            else:
                s = IR.sphere(g, o, d, t_max)
                f = self.sphere_fragile(g, o, d, t_max)
            parts.append(s)
            ts.append(np.where(s["hit"], s["t"], np.inf))
            raws.append(s["t"]); frs.append(f)
        out = {k: np.zeros((m,) + parts[0][k].shape[1:]) for k in FIELDS} if parts else {k: np.zeros((m, 3)) for k in FIELDS}
        if not parts:
            out.update(hit=np.zeros(m, bool), prim=np.full(m, -1, np.int64), fragile=np.zeros(m, bool))
            return out
        ts = np.stack(ts)
        prim = np.argmin(ts, axis=0)
        tb = ts[prim, np.arange(m)]
        hit = np.isfinite(tb)
        fragile = np.zeros(m, bool)
        with np.errstate(all="ignore"):
            # a doubtful candidate counts unless it lies clearly behind the nearest hit, or behind the origin: t <= 0 is a miss in binary32 as well,
            # since the reference's own test (triangle.rs:252-268, sphere.rs:99-110) asks for t above a rigorous bound on its error
            for raw, f in zip(raws, frs):
                fragile |= f & ~(raw > tb * (1.0 + 1.0e-4)) & ~(raw <= 0.0)
            if len(parts) > 1:                        # the two nearest within rounding of each other: brute force and the BVH may order them otherwise
                two = np.partition(ts, 1, axis=0)[:2]
                fragile |= hit & (two[1] - two[0] <= 1.0e-5 * np.abs(two[0]))
        for i, s in enumerate(parts):
            sel = hit & (prim == i)
            for k in FIELDS:
                out[k][sel] = s[k][sel]
        out.update(hit=hit, prim=np.where(hit, prim, -1), fragile=fragile)
        return out

    def occluded(self, o, d, t_max=None):
        """Scene::intersect_test -> occluded, fragile; t_max per ray, a shadow ray's (1 - 0.0001) by default"""
        m = len(o)
        t_max = np.full(m, SHADOW_T_MAX) if t_max is None else np.asarray(t_max, np.float64)
        occ, firm, doubt = np.zeros(m, bool), np.zeros(m, bool), np.zeros(m, bool)
        for g in self.geo:
            if g.kind == "tri":
                h = g.hit_test(o, d, t_max)
                with np.errstate(all="ignore"):       # behind the origin or clearly beyond t_max: a miss in binary32 as well (see intersect)
                    hit, f = ~h["miss"], h["fragile"] & ~(h["t"] <= 0.0) & ~(h["t"] > t_max * (1.0 + 1.0e-4))
            else:
                hit, f = g.intersect(o, d, t_max)[0], self.sphere_fragile(g, o, d, t_max)
            occ |= hit
            firm |= hit & ~f
            doubt |= f
        return occ, doubt & ~firm

    def unoccluded(self, S, p1_p, p1_perr, p1_n):
        """VisibilityTester::unoccluded (light/mod.rs:82-84) through spawn_ray_to_hit (interaction.rs:48-58): both ends are offset"""
        origin = R.offset_ray_origin(S["p"], S["p_err"], S["n"], p1_p - S["p"])
        target = R.offset_ray_origin(p1_p, p1_perr, p1_n, origin - p1_p)
        occ, fragile = self.occluded(origin, target - origin)
        return ~occ, fragile

    def spawn(self, S, w):                            # interaction.rs:22-30
        return R.offset_ray_origin(S["p"], S["p_err"], S["n"], w), w

    def emitted(self, S, prim, w):
        """SurfaceInteraction::emitted_radiance (interaction.rs:175-180), DiffuseAreaLight::emitted_radiance (diffuse.rs:44-50) -> L, fragile"""
        c = dot(S["n"], w)
        e = self.emit[np.maximum(prim, 0)] * (prim >= 0)[:, None]
        return np.where((c > 0.0)[:, None], e, 0.0), ~black(e) & (np.abs(c) <= 1.0e-6 * R.norm(w))

    def environment(self, d):
        """Scene::environment_emitted_radiance (scene/mod.rs:59-64): the sum over all lights; only infinite lights return any (infinite.rs:156-164)"""
        out = np.zeros((len(d), 3))
        for l in self.lights:
            if l["kind"] == "infinite" and len(d):
                out = out + l["env"].Le(d)[0]
        return out

    # ---- compute_scattering_functions (interaction.rs:111-121) and the materials
    def scattering(self, mat, S, multiple, diff):
        """-> Bsdf (None where the material refuses, glass.rs:66-67), its eta (Bsdf::new's argument), fragile, the texture differentials and
        whether they are fragile (None in a scene without textures: they reach nothing but textures and the children of specular bounces)"""
        n = len(S["p"])
        fragile = np.zeros(n, bool)
        td = ftd = None
        if self.textured:
            td, ftd = IR.tex_differentials(S, np.ones(n), diff["rxo"], diff["ryo"], diff["rxd"], diff["ryd"])
        m = self.materials[mat]
        eta = float(m.s0) if m.type == A.FTN_MAT_GLASS else 1.0
        if self.tex.is_textured(mat):
            rows = np.concatenate([S["uv"], td["dudx"][:, None], td["dvdx"][:, None], td["dudy"][:, None], td["dvdy"][:, None]], axis=1)
            res, f = self.tex.resolve(mat, rows)
            if m.type != A.FTN_MAT_MATTE or np.any(res[:, 9] != 0.0):
                raise NotImplementedError("textured parameters: only a matte Kd")
            r = np.maximum(res[:, 3:6], 0.0)          # matte.rs:36-52
            assert not black(r).any(), "a black texel changes the number of lobes per row"
            lobes = [B.Lobe("lambert", r)]
            fragile = ftd | f
        else:
            lobes = B.material_lobes(KIND[m.type], multiple, **material_keywords(m))
        if lobes is None:
            return None, eta, fragile, td, ftd
        return B.Bsdf(lobes, S["n"], S["ns"], S["s_dpdu"]), eta, fragile, td, ftd


# ---------------------------------------------------------------- the integrators
class Integrate:
    """one render of `n` camera samples.  kind: "path" (max_depth, rr_threshold) | "direct" | "whitted" (max_depth)"""

    def __init__(self, scene, cam_desc, spp, seed, px, py, sample, kind, max_depth, rr_threshold=1.0):
        self.sc, self.kind, self.max_depth, self.rr = scene, kind, int(max_depth), float(np.float32(rr_threshold))
        n = len(px)
        self.n = n
        self.rng = Rng(seed, px, py, sample)
        self.fragile = np.zeros(n, bool)
        self.rays_closest, self.rays_any = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.error = 0
        every = np.arange(n)
        # get_camera_sample, sampler/mod.rs:43-51: p_film (2), p_lens (2), time (1); pixel + u in binary32
        u = self.rng.f2(every)
        self.p_film = (np.stack([px, py], axis=1).astype(np.float32) + u.astype(np.float32)).astype(np.float32)
        lens = self.rng.f2(every)
        time = self.rng.f(every)
        cam = IR.camera(cam_desc, spp, np.concatenate([self.p_film.astype(np.float64), lens, time[:, None]], axis=1))      # integrator/mod.rs:246-251
        self.fragile |= cam["fragile"]
        self.ray_weight = np.ones(n, np.float32)
        ray = dict(o=cam["o"], d=cam["d"], rxo=cam["rxo"], ryo=cam["ryo"], rxd=cam["rxd"], ryd=cam["ryd"])
        with np.errstate(all="ignore"):
            self.L = self.path(every, ray) if kind == "path" else self.direct(every, ray, 0)

    def flag(self, idx, f):
        self.fragile[idx] |= f

    # ---- integrator/mod.rs:307-395
    def estimate_direct(self, idx, S, bsdf, u_scattering, li, u_light, whitted=False):
        sc = self.sc
        light = sc.lights[li]
        n = len(idx)
        delta = light["kind"] in ("point", "distant")
        wo, ns = S["wo"], S["ns"]
        if not delta and not whitted:                 # :346 (computed first here: its direction is what the light's pdf is asked for)
            m2 = []
            ok2, f2, wi2, pdf2, _ = bsdf.sample_f(wo, u_scattering, NONSPEC, m2)
            f2 = f2 * np.abs(dot(wi2, ns))[:, None]                                          # :348
            use2 = ok2 & ~black(f2)                                                          # :351
            self.flag(idx, close(m2, n) | (ok2 & tiny(f2)))
        else:
            ok2 = use2 = np.zeros(n, bool)
            wi2 = ns
        # R.evaluate answers the sample and the pdf of a given direction in one call and merges their flags: where no direction is asked for, hand it
        # one whose answer is firm (towards the middle of an area light's shape)
        spare = R.normalize(light["shape"].centre - S["p"]) if light["kind"] == "area" else ns
        wi_in = np.where(use2[:, None], wi2, spare)
        rows = np.concatenate([S["p"], S["p_err"], S["n"], np.zeros((n, 1)), wi_in, u_light], axis=1)
        ev = R.evaluate(light, rows)                  # :321 and :358
        if bsdf.num_components(B.ALL if whitted else NONSPEC) > 0:      # without a matching lobe f is black whatever the light answers
            fl = ev["fragile"]
            if light["kind"] == "area" and light["shape"].kind == "sph":
                # _light_ref flags a root within 1e-4 of the sphere's size of 0, which is every reference point ON the emitting sphere (the furnace);
                # the finer predicate of SceneRef.sphere_fragile instead, on the two rays shapes/mod.rs:55-66 intersects, and the emission's cosine
                fl = np.abs(dot(ev["p1_n"], -ev["wi"])) <= 1.0e-5
                for w in (wi_in, ev["wi"]):
                    fl = fl | sc.sphere_fragile(light["shape"], R.offset_ray_origin(S["p"], S["p_err"], S["n"], w), w, np.full(n, np.inf))
            self.flag(idx, fl)
        radiance = np.zeros((n, 3))
        pdf, rad, wi = ev["pdf"], ev["radiance"], ev["wi"]
        if whitted:                                   # whitted.rs:47-55
            gate1 = ~(black(rad) | (pdf == 0.0)) & ~np.isnan(pdf)
            flags = B.ALL
        else:
            gate1 = (pdf > 0.0) & ~black(rad)         # :322
            flags = NONSPEC
        m1 = []
        f = bsdf.f(wo, wi, flags, m1)
        cos = np.abs(dot(wi, ns))
        if not whitted:
            f = f * cos[:, None]                      # :324-326
            scattering_pdf = bsdf.pdf(wo, wi, NONSPEC)                                       # :328
        self.flag(idx, gate1 & (close(m1, n) | tiny(f) | tiny(pdf)))
        gate2 = gate1 & ~black(f)                     # :332
        k = np.flatnonzero(gate2)
        if len(k):
            vis, fv = sc.unoccluded(rows_of(S, k), ev["p1_p"][k], ev["p1_perr"][k], ev["p1_n"][k])
            self.rays_any[idx[k]] += 1
            self.flag(idx[k], fv)
            if whitted:
                c = f[k] * rad[k] * cos[k][:, None] / pdf[k][:, None]
            elif delta:
                c = f[k] * rad[k] / pdf[k][:, None]                                          # :334
            else:
                c = f[k] * rad[k] * power_heuristic(pdf[k], scattering_pdf[k])[:, None] / pdf[k][:, None]      # :336-337
            radiance[k] += np.where(vis[:, None], c, 0.0)
        if not delta and not whitted:                 # :345-392
            light_pdf = ev["pdf_in"]
            go = use2 & ~(light_pdf == 0.0)           # :359
            k = np.flatnonzero(go)
            if len(k):
                Sk = rows_of(S, k)
                o, d = sc.spawn(Sk, wi2[k])           # :364
                H = sc.intersect(o, d)                # :367
                self.rays_closest[idx[k]] += 1
                self.flag(idx[k], H["fragile"] | tiny(light_pdf[k]))
                same = H["hit"] & (sc.light_of_prim[np.maximum(H["prim"], 0)] == li)         # :369-381
                inc, fe = sc.emitted(H, np.where(same, H["prim"], -1), -wi2[k])
                self.flag(idx[k], fe)
                if light["kind"] == "infinite":       # :384
                    miss = ~H["hit"]
                    inc[miss] = light["env"].Le(d[miss])[0] if miss.any() else inc[miss]
                w = power_heuristic(pdf2[k], light_pdf[k])                                   # :362
                c = f2[k] * inc * w[:, None] / pdf2[k][:, None]
                radiance[k] += np.where(black(inc)[:, None], 0.0, c)                         # :387-389
        return radiance

    def uniform_sample_one_light(self, idx, S, bsdf):                                        # integrator/mod.rs:289-305
        n_lights = len(self.sc.lights)
        n = len(idx)
        out = np.zeros((n, 3))
        if n_lights == 0:                             # before any draw
            return out
        x = self.rng.f(idx) * n_lights
        num = np.minimum(np.floor(x), n_lights - 1).astype(np.int64)
        self.flag(idx, (np.abs(x - np.round(x)) <= 1.0e-6 * n_lights) & (n_lights > 1))
        u_light = self.rng.f2(idx)
        u_scattering = self.rng.f2(idx)
        for li in range(n_lights):
            k = np.flatnonzero(num == li)
            if len(k):
                out[k] = n_lights * self.estimate_direct(idx[k], rows_of(S, k), sub_bsdf(bsdf, k), u_scattering[k], li, u_light[k])
        return out

    # ---- integrator/path.rs:25-95
    def path(self, every, ray):
        sc = self.sc
        n = self.n
        L, beta = np.zeros((n, 3)), np.ones((n, 3))
        bounces, specular = np.zeros(n, np.int64), np.zeros(n, bool)
        o, d = ray["o"].copy(), ray["d"].copy()
        alive = np.ones(n, bool)
        self.bounces_at_end = bounces
        self.roulette_cut = np.zeros(n, bool)
        while alive.any():
            idx = np.flatnonzero(alive)
            S = sc.intersect(o[idx], d[idx])          # :42
            self.rays_closest[idx] += 1
            self.flag(idx, S["fragile"])
            add = (bounces[idx] == 0) | specular[idx]                                        # :45
            le, fe = sc.emitted(S, S["prim"], -d[idx])
            le = np.where(S["hit"][:, None], le, sc.environment(d[idx]))
            L[idx] += np.where(add[:, None], beta[idx] * le, 0.0)
            self.flag(idx, add & S["hit"] & fe)
            stop = ~S["hit"] | (bounces[idx] >= self.max_depth)                              # :54
            alive[idx[stop]] = False
            mats = sc.mat[np.maximum(S["prim"], 0)]
            for mat in np.unique(mats[~stop]):
                k = np.flatnonzero(~stop & (mats == mat))
                ik = idx[k]
                Sk = rows_of(S, k)
                if mat < 0:                           # :77-81: the null material, without `bounces += 1`
                    o[ik], d[ik] = sc.spawn(Sk, d[ik])
                    continue
                bsdf, _, fr, _, _ = sc.scattering(int(mat), Sk, True, {c: ray[c][ik] for c in ("rxo", "ryo", "rxd", "ryd")})      # :59, the camera's differential as it was (:73)
                self.flag(ik, fr)
                if bsdf is None:
                    self.error = A.FTN_ERR_UNSUPPORTED
                    alive[ik] = False
                    continue
                if bsdf.num_components(NONSPEC) > 0:                                         # :62-65
                    L[ik] += beta[ik] * self.uniform_sample_one_light(ik, Sk, bsdf)
                m = []
                ok, f, wi, pdf, typ = bsdf.sample_f(-d[ik], self.rng.f2(ik), B.ALL, m)       # :68-69
                self.flag(ik, close(m, len(ik)) | (ok & tiny(f)))
                go = ok & ~black(f)                   # :70
                alive[ik[~go]] = False
                g = ik[go]
                beta[g] *= f[go] * np.abs(dot(wi[go], Sk["ns"][go]))[:, None] / pdf[go][:, None]                                 # :71
                specular[g] = (typ[go] & B.SPECULAR) != 0
                o[g], d[g] = sc.spawn(rows_of(Sk, go), wi[go])
                top = beta[g].max(axis=1)
                late = bounces[g] > 3
                self.flag(g, late & (np.abs(top - self.rr) <= 1.0e-6))
                rr = g[(top < self.rr) & late]        # :84
                if len(rr):
                    q = np.maximum(float(np.float32(0.05)), 1.0 - beta[rr].max(axis=1))      # :85
                    u = self.rng.f(rr)
                    self.flag(rr, np.abs(u - q) <= 1.0e-6)
                    cut = u < q                       # :86
                    alive[rr[cut]] = False
                    self.roulette_cut[rr[cut]] = True
                    beta[rr[~cut]] /= (1.0 - q[~cut])[:, None]                               # :89
                    g = np.setdiff1d(g, rr[cut], assume_unique=True)
                bounces[g] += 1                       # :92
        return L

    # ---- integrator/direct_lighting.rs:50-106 (UniformSampleOne), integrator/whitted.rs:20-71
    def direct(self, idx, ray, depth):
        sc = self.sc
        whitted = self.kind == "whitted"
        n = len(idx)
        L = np.zeros((n, 3))
        S = sc.intersect(ray["o"], ray["d"])
        self.rays_closest[idx] += 1
        self.flag(idx, S["fragile"])
        miss = ~S["hit"]
        L[miss] = sc.environment(ray["d"][miss])      # direct_lighting.rs:54-56
        mats = sc.mat[np.maximum(S["prim"], 0)]
        for mat in np.unique(mats[S["hit"]]):
            k = np.flatnonzero(S["hit"] & (mats == mat))
            ik = idx[k]
            Sk = rows_of(S, k)
            if mat < 0:                               # unimplemented!(), direct_lighting.rs:98 / whitted.rs:63
                self.error = A.FTN_ERR_UNSUPPORTED
                continue
            diff = {c: ray[c][k] for c in ("rxo", "ryo", "rxd", "ryd")}
            bsdf, eta, fr, td, ftd = sc.scattering(int(mat), Sk, False, diff)
            self.flag(ik, fr)
            if bsdf is None:
                self.error = A.FTN_ERR_UNSUPPORTED
                continue
            if whitted:                               # whitted.rs:41-56: every light, one 2D sample each; no emission
                for li in range(len(sc.lights)):
                    L[k] += self.estimate_direct(ik, Sk, bsdf, None, li, self.rng.f2(ik), whitted=True)
            else:
                le, fe = sc.emitted(Sk, S["prim"][k], Sk["wo"])                              # direct_lighting.rs:69
                self.flag(ik, fe)
                L[k] += le
                L[k] += self.uniform_sample_one_light(ik, Sk, bsdf)
            if depth + 1 < self.max_depth:            # direct_lighting.rs:93-96
                for reflect, flags in ((1.0, B.REFLECTION | B.SPECULAR), (0.0, B.TRANSMISSION | B.SPECULAR)):
                    u = self.rng.f2(ik)               # drawn before the match, integrator/mod.rs:53 / :113
                    m = []
                    ok, f, wi, pdf, _ = bsdf.sample_f(Sk["wo"], u, flags, m)
                    if not ok.any():
                        continue
                    self.flag(ik, ok & close(m, len(ik)))
                    cos = np.abs(dot(wi, Sk["ns"]))
                    go = ok & ~(cos == 0.0)           # :55 / :115
                    g = np.flatnonzero(go)
                    if not len(g):
                        continue
                    Sg = rows_of(Sk, g)
                    co, cd = sc.spawn(Sg, wi[g])
                    child = dict(o=co, d=cd, rxo=ray["rxo"][k][g], ryo=ray["ryo"][k][g], rxd=ray["rxd"][k][g], ryd=ray["ryd"][k][g])
                    if td is not None:                # :59-83 / :119-164
                        tdg = {c: v[g] for c, v in td.items()}
                        sp, fs = IR.specular(Sg, tdg, np.ones(len(g)), diff["rxd"][g], diff["ryd"][g], wi[g], np.full(len(g), eta), np.full(len(g), reflect))
                        child.update(sp)
                        self.flag(ik[g], fs | ftd[g])
                    li = self.direct(ik[g], child, depth + 1)
                    L[k[g]] += f[g] * li * cos[g][:, None] / pdf[g][:, None]                 # :93 / :174
        return L


def render(builder, cam, res, spp, seed, kind, max_depth, rr_threshold=1.0, first=0, count=0, area_order=None):
    """every camera sample of a full-crop film of radius 0.5 (its sample bounds are the pixels), pixels row-major, samples increasing ->
    dict(px, py, sample, p_film [n, 2] binary32, L [n, 3], ray_weight, fragile, rays_closest, rays_any, error, roulette_cut)"""
    count = count or spp - first
    ys, xs, ss = np.meshgrid(np.arange(res[1]), np.arange(res[0]), np.arange(first, first + count), indexing="ij")
    px, py, s = xs.ravel(), ys.ravel(), ss.ravel()
    scene = builder if isinstance(builder, SceneRef) else SceneRef(builder, area_order)
    it = Integrate(scene, cam.desc, spp, seed, px, py, s, kind, max_depth, rr_threshold)
    return dict(px=px, py=py, sample=s, p_film=it.p_film, L=it.L, ray_weight=it.ray_weight, fragile=it.fragile, rays_closest=it.rays_closest,
                rays_any=it.rays_any, error=it.error, roulette_cut=getattr(it, "roulette_cut", np.zeros(len(px), bool)), draws=it.rng.draws)
