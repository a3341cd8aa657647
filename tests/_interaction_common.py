"""Shared by tests/test_interaction_cpu.py (the oracle) and tests/test_interaction.py (the device): the one-to-four-primitive scenes and the
cameras, the rows fed to the interaction and camera hooks (ftn_test_interaction / orc_test_interaction, ftn_test_camera / orc_test_camera),
and the property checks, so that both sides face the same seeds and the same bounds.  Every bound below follows from the
number formats or from reasoning written next to it; none comes from what a library returned."""
import ctypes as C

import numpy as np

import _light_ref as R
from _light_common import TRI_VARIANTS, above, below, same_bits_or_both_nan, unit
from _rows import run_rows
from fountain_amd import PerspectiveCamera, SceneBuilder, Transform, _abi as A

f32 = np.float32
EPS = R.EPS
NIN, NOUT = A.FTN_TEST_INTERACTION_IN, A.FTN_TEST_INTERACTION_OUT
CIN, COUT = A.FTN_TEST_CAMERA_IN, A.FTN_TEST_CAMERA_OUT
COL = dict(hit=0, t=1, bary=slice(2, 5), p=slice(5, 8), p_err=slice(8, 11), n=slice(11, 14), time=14, wo=slice(15, 18), ns=slice(18, 21),
           s_dpdu=slice(21, 24), mat=24, light=25, uv=slice(26, 28), dpdu=slice(28, 31), dpdv=slice(31, 34), dndu=slice(34, 37), dndv=slice(37, 40),
           dpdx=slice(40, 43), dpdy=slice(43, 46), dudx=46, dvdx=47, dudy=48, dvdy=49, spawn_o=slice(50, 53), spawn_tmax=53,
           rxo=slice(54, 57), ryo=slice(57, 60), rxd=slice(60, 63), ryd=slice(63, 66))
DSI_COLUMNS = ["p", "p_err", "n", "time", "wo", "ns", "s_dpdu", "mat", "light"]
CAM = dict(o=slice(0, 3), d=slice(3, 6), t_max=6, time=7, rxo=slice(8, 11), ryo=slice(11, 14), rxd=slice(14, 17), ryd=slice(17, 20))
# the rays of a triangle's edge table that the triangle test cannot decide (undefined_by_the_reference): 4 of the 38 rays of edge_rays() -- an
# origin 3e20 off the plane on either side, a direction of length 3e20, a zero direction -- each repeated as often as the others or (the every-third
# subsets) less.  No more rows than that share may fall under the predicate, none of a sphere's and none of the random rows
MAX_UNDEFINED_SHARE = 4.0 / 38.0

# ---- measured tolerances.  Metric: |got - want| / max(|want|, floor) per component, floor per column group
# (tests/_interaction_ref.py: UNIT, POSITIONS, VECTORS), rows flagged fragile left out.  Measured with the libm oracle against the binary64
# restatement (tests/_interaction_ref.py) on the CPU, per configuration of test_oracle_matches_the_restatement: (99.9th percentile, maximum).
# The bounds are 4 x each configuration's own measurement.  What sets the maxima: dpdx / dudy of auxiliary rays near grazing, whose plane
# intersection cancels the hit point's coordinates (1e4 on tri_far); on sph_scaled the quotient by n . rxd with an n that is not the surface's.
MEASURED = {
    "tri_plain": (1.74e-3, 0.43), "tri_normals": (1.74e-3, 0.43), "tri_normals_against": (1.74e-3, 0.43), "tri_reversed": (1.74e-3, 0.43),
    "tri_mirrored": (1.71e-3, 0.193), "tri_uv": (1.66e-3, 0.43), "tri_uv_degenerate": (2.10e-3, 1.8), "tri_uv_degenerate_normals": (2.10e-3, 1.8),
    "tri_uv_degenerate_one_normal": (2.10e-3, 1.8), "tri_normals_uv": (1.66e-3, 0.43), "tri_tangents": (1.74e-3, 0.43),
    "tri_tangents_normals": (1.66e-3, 0.43), "tri_tangent_along_normal": (1.74e-3, 0.43), "tri_sliver": (1.29e-5, 6.42e-4),
    "tri_far": (1.09e-2, 19.9), "tri_pair": (1.62e-3, 0.391), "sph_full": (3.48e-3, 0.295), "sph_partial": (3.60e-3, 0.52),
    "sph_reversed": (3.46e-3, 0.295), "sph_scaled": (7.34e-3, 11.9), "sph_tiny": (5.35e-3, 1.09), "sph_huge": (3.02e-3, 0.331),
}
TOLERANCE = {k: (4.0 * a, 4.0 * b) for k, (a, b) in MEASURED.items()}
MEASURED_FRAGILE_SHARE = 0.0032                 # largest share of rows left out in one configuration (sph_scaled), libm oracle
MEASURED_CAMERA = 1.02e-4                       # far_rotated: the maximum over every output, rows and samples-per-pixel count
TOL_CAMERA = 4.0 * MEASURED_CAMERA
MAX_FRAGILE_SHARE = 0.005
# the share of the random rows whose origin lies on the primitive itself: a root at the origin is decided by the reference's error intervals, which
# are not restated, so each such row on a sphere is left out (the bit-for-bit comparison with the device runs with 20 % of them)
ON_SURFACE = 0.002

# ---------------------------------------------------------------- configurations
TRI_P = [(-1.0, -1.0, 0.0), (1.0, -1.0, 0.25), (0.0, 1.0, 0.5)]
TRI_N = [(0.1, 0.2, 1.0), (-0.2, 0.1, 0.9), (0.3, -0.1, 1.1)]
TRI_UV = [(0.1, 0.2), (0.9, 0.15), (0.3, 0.85)]
ONE_N = [(0.1, 0.2, 1.0)] * 3
TRIANGLES = {
    "tri_plain": dict(P=TRI_P),
    "tri_normals": dict(P=TRI_P, N=TRI_N),
    "tri_normals_against": dict(P=TRI_P, N=[(-a, -b, -c) for a, b, c in TRI_N]),                 # the winding's normal has z > 0
    "tri_reversed": dict(P=TRI_P, N=TRI_N, reverse=True),
    "tri_mirrored": dict(P=TRI_P, mirror=True),                                                  # a handedness-swapping transform: GF_FLIP
    "tri_uv": dict(P=TRI_P, uv=TRI_UV),
    "tri_uv_degenerate": dict(P=TRI_P, uv=[(0.5, 0.5), (0.5 + 5.0e-5, 0.5), (0.5, 0.5 + 5.0e-5)]),  # |determinant| = 2.5e-9 < 1e-8, not 0
    "tri_uv_degenerate_normals": dict(P=TRI_P, N=TRI_N, uv=[(0.5, 0.5)] * 3),
    "tri_uv_degenerate_one_normal": dict(P=TRI_P, N=ONE_N, uv=[(0.5, 0.5)] * 3),                   # dn == 0
    "tri_normals_uv": dict(P=TRI_P, N=TRI_N, uv=TRI_UV),
    "tri_tangents": dict(P=TRI_P, S=[(1.0, 0.1, 0.0), (0.9, -0.1, 0.2), (1.1, 0.0, -0.1)]),
    "tri_tangents_normals": dict(P=TRI_P, N=TRI_N, uv=TRI_UV, S=[(1.0, 0.1, 0.0), (0.9, -0.1, 0.2), (1.1, 0.0, -0.1)]),
    "tri_tangent_along_normal": dict(P=TRI_P, N=ONE_N, S=ONE_N),                                  # ns and ss are the same bits: len2(ts) == 0
    "tri_sliver": dict(P=[(0.0, 0.0, 0.0), (1.0e-6, 0.0, 0.0), (0.0, 2.0e-6, 0.0)], N=[(0.0, 0.1, 1.0), (0.1, 0.0, 1.0), (0.0, 0.0, 1.0)]),   # area 1e-12
    "tri_far": dict(P=[(10000.0, 12000.0, 9000.0), (12500.0, 10000.0, 9500.0), (10500.0, 13000.0, 11000.0)], N=TRI_N, uv=TRI_UV),
    "tri_pair": dict(P=TRI_P + [(2.0, 1.0, -0.5)], N=TRI_N + [(0.0, 0.3, 1.0)], uv=TRI_UV + [(0.95, 0.9)], indices=[0, 1, 2, 2, 1, 3]),       # one shared edge
}
SPHERES = {
    "sph_full": dict(radius=1.5, at=(0.5, -1.0, 2.0)),
    "sph_partial": dict(radius=1.0, at=(0.5, -1.0, 2.0), zmin=-0.3, zmax=0.7, phimax=250.0),
    "sph_reversed": dict(radius=1.5, at=(0.5, -1.0, 2.0), reverse=True),
    "sph_scaled": dict(radius=1.0, at=(0.5, -1.0, 2.0), rotate=(35.0, (1.0, 2.0, 3.0)), scale=(1.5, 0.7, 1.1)),
    "sph_tiny": dict(radius=1.0e-3, at=(0.004, -0.002, 0.003)),          # (near the world's origin: at a distance of 2 the translation alone costs binary32 1e-4 of this radius)
    "sph_huge": dict(radius=1.0e4, at=(0.5, -1.0, 2.0)),
}
TRANSLATED_SPHERES = ["sph_full", "sph_partial", "sph_reversed", "sph_tiny", "sph_huge"]
ALL_NAMES = list(TRIANGLES) + list(SPHERES)
# the bounced differentials of every configuration but the sliver: its 2 x 2 system is singular (|determinant| 2e-12 < 1e-10), every differential
# is zero and there is no neighbouring ray to compare (check_texture_differentials asserts the zeros)
BOUNCE_NAMES = [k for k in ALL_NAMES if k != "tri_sliver"]
# Exact refraction takes a unit normal: the transmitted differential is compared where dndx is perpendicular to ns, i.e. on flat triangles (dndx = 0) and
# on spheres under a translation.  (A triangle's dndu is the difference of its UNNORMALISED vertex normals times the barycentric determinant, a
# sphere's under a non-uniform scale goes through transform_normal: neither is the derivative of the unit normal.  Reflection, which is compared
# with -w + 2 (w . n) n for the n the formula itself uses, takes every configuration.)
TRANSMIT_NAMES = ["tri_plain", "tri_mirrored", "tri_uv", "tri_uv_degenerate", "tri_tangents", "tri_uv_degenerate_one_normal", "tri_tangent_along_normal", "tri_far"] + TRANSLATED_SPHERES
# the share of sph_scaled's rows of check_spawned_ray_leaves (seed 72) on which the returned n and the surface's own normal disagree about wi's side: measured
# on the libm oracle; the rows are seeded and the normals differ by tens of degrees, so the count moves by a few rows at most between builds
SCALED_SPHERE_DISAGREEMENT = 0.2878


def variants_of(name):
    return list(TRI_VARIANTS) if name in TRIANGLES else ["default"]


def build(be, name, variant="default"):
    b = SceneBuilder(be)
    b.material("matte", Kd=(0.4, 0.5, 0.6))
    b.attribute_begin()
    if name in TRIANGLES:
        s = TRIANGLES[name]
        if s.get("mirror"):
            b.scale(1.0, 1.0, -1.0)
        if s.get("reverse"):
            b.reverse_orientation()
        if name != "tri_uv":                          # one configuration without an area light: light = -1
            b.area_light_source("diffuse", L=(5.0, 4.0, 3.0))
        b.shape("trianglemesh", P=s["P"], N=s.get("N"), uv=s.get("uv"), S=s.get("S"), indices=s.get("indices", [0, 1, 2]))
        b.attribute_end()
        if variant == "dense":                        # a sphere far from every ray aimed at the triangles: the dense `geom` array is resident
            b.attribute_begin(); b.translate((300.0, -200.0, 100.0)); b.shape("sphere", radius=1.0); b.attribute_end()
        return b
    s = SPHERES[name]
    b.translate(s["at"])
    if "rotate" in s:
        b.rotate(*s["rotate"])
    if "scale" in s:
        b.scale(*s["scale"])
    if s.get("reverse"):
        b.reverse_orientation()
    b.shape("sphere", radius=s["radius"], zmin=s.get("zmin", -s["radius"]), zmax=s.get("zmax", s["radius"]), phimax=s.get("phimax", 360.0))
    b.attribute_end()
    return b


class Tri(R.Triangle):
    kind = "tri"

    def __init__(self, b, tri):
        super().__init__(b, tri)
        idx = np.concatenate(b.tri_indices)[tri]
        mesh = b.meshes[int(np.concatenate(b.tri_mesh)[tri])]
        self.has_uv = bool(mesh.has_uvs)
        self.s = np.concatenate(b.S).astype(np.float64)[idx] if mesh.has_tangents else None
        self.centre = self.p.mean(axis=0)
        self.radius = float(np.max(np.linalg.norm(self.p - self.centre, axis=1)))
        self.ng = R.normalize(np.cross(self.p[1] - self.p[0], self.p[2] - self.p[0]))
        duv02, duv12 = self.uv[0] - self.uv[2], self.uv[1] - self.uv[2]
        self.uv_det = float(f32(f32(duv02[0]) * f32(duv12[1])) - f32(f32(duv02[1]) * f32(duv12[0])))
        self.degenerate_uv = abs(self.uv_det) < 1.0e-8

    def t_of(self, o, d):
        with np.errstate(all="ignore"):
            return R.dot(self.p[0] - o, self.ng) / R.dot(d, self.ng)

    def surface(self, rng, n):
        b = rng.dirichlet((1.0, 1.0, 1.0), n)
        return b @ self.p


class Sph(R.Sphere):
    kind = "sph"

    def __init__(self, s):
        super().__init__(s)
        self.centre = R.tf_point(self.o2w, np.zeros(3))
        self.radius = self.r * float(np.max(np.linalg.norm(self.o2w[:3, :3], axis=0)))

    def roots(self, o, d):
        with np.errstate(all="ignore"):
            oo, dd = R.tf_point(self.w2o, o), R.tf_vector(self.w2o, d)
            a, b, c = R.dot(dd, dd), 2.0 * R.dot(dd, oo), R.dot(oo, oo) - self.r ** 2
            disc = np.sqrt(np.maximum(b * b - 4.0 * a * c, 0.0))
            return (-b - disc) / (2.0 * a), (-b + disc) / (2.0 * a)

    def t_of(self, o, d):
        t0, t1 = self.roots(o, d)
        return np.where(t0 > 1.0e-4 * self.radius, t0, t1)

    def surface(self, rng, n):
        return R.tf_point(self.o2w, self.r * unit(rng, n))


def geometry(b):
    """the primitives of a SceneBuilder in the order it holds them (what ftn_prim indexes), from the builder's own arrays"""
    out = []
    for p in b.prims:
        if p[0] == "trirange":
            out += [Tri(b, p[1] + k) for k in range(p[2])]
        else:
            out.append(Sph(b.spheres[p[1]]))
    return out


class Hook:
    """the interaction hook of one backend on one configuration.  Rows carry the BUILDER's primitive index; raw() turns it into the BVH's through the
    order the library reports (check_primitive_mapping tests that order with rays).  FTN_SREC is read when the scene is created."""

    def __init__(self, be, name, variant="default", monkeypatch=None):
        self.be, self.name, self.variant = be, name, variant
        self.builder = build(be, name, variant)
        knobs = TRI_VARIANTS.get(variant, {})
        if be.is_oracle or monkeypatch is None:
            assert be.is_oracle or not knobs
            self.scene = self.builder.create_scene()
        else:
            with monkeypatch.context() as mp:
                mp.delenv("FTN_SREC", raising=False)
                for k, v in knobs.items():
                    mp.setenv(k, v)
                self.scene = self.builder.create_scene()
        self.fn = be.lib.orc_test_interaction if be.is_oracle else be.lib.ftn_test_interaction
        self.fn.argtypes = A.TEST_INTERACTION_ARGTYPES
        self.fn.restype = C.c_int
        self.geo = geometry(self.builder)
        self.targets = [g for g in self.geo if not (variant == "dense" and g.kind == "sph")]
        self.order = self.scene.nodes()[1].astype(np.int64)         # BVH position -> builder index
        self.to_bvh = np.argsort(self.order)

    def raw(self, rows, bvh_indices=False):
        rows = np.array(rows, f32, order="C").reshape(-1, NIN)
        if not bvh_indices:
            rows[:, 8:9].view(np.int32)[:, 0] = self.to_bvh[rows[:, 8:9].view(np.int32)[:, 0]]
        return run_rows(self.be, lambda pin, n, pout: self.fn(self.scene.handle, pin, n, pout), rows, NIN, NOUT)

    def __call__(self, rows):
        return unpack(self.raw(rows))


def unpack(out):
    o = {k: out[:, c].astype(np.float64) for k, c in COL.items()}
    o["hit"] = out[:, 0] != 0.0
    o["mat"], o["light"] = out[:, 24:25].view(np.int32)[:, 0], out[:, 25:26].view(np.int32)[:, 0]
    return o


# ---------------------------------------------------------------- rows
def make_rows(o, d, prim, t_max=np.inf, time=0.0, has=0.0, rxo=0.0, ryo=0.0, rxd=0.0, ryd=0.0, wi=(0.0, 0.0, 1.0), eta=1.5, reflect=1.0):
    o, d = np.atleast_2d(np.asarray(o, np.float64)), np.atleast_2d(np.asarray(d, np.float64))
    m = max(len(o), len(d), np.size(prim), np.size(t_max), len(np.atleast_2d(wi)), len(np.atleast_2d(rxd)), np.size(has), np.size(eta), np.size(reflect))
    rows = np.zeros((m, NIN), f32)
    with np.errstate(all="ignore"):
        rows[:, 0:3], rows[:, 3:6], rows[:, 6], rows[:, 7] = o, d, t_max, time
        rows[:, 8:9].view(np.int32)[:, 0] = prim
        rows[:, 9], rows[:, 10:13], rows[:, 13:16], rows[:, 16:19], rows[:, 19:22] = has, rxo, ryo, rxd, ryd
        rows[:, 22:25], rows[:, 25], rows[:, 26] = wi, eta, reflect
    return rows


def prim_of(rows):
    return rows[:, 8:9].view(np.int32)[:, 0]


def perpendicular(d):
    a = np.where((np.abs(d[:, 0:1]) > 0.9), np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    u = R.normalize(np.cross(d, a))
    return u, np.cross(d, u)


def differential(o, d, eps, lens=0.0, rng=None):
    """the auxiliary rays a camera would give a ray (o, d): directions eps radians off along two perpendicular axes, origins at o or, with a lens, beside it"""
    u, v = perpendicular(d)
    eps = np.broadcast_to(np.asarray(eps, np.float64), (len(d),))[:, None]
    off = lens * unit(rng, len(d)) if rng is not None else 0.0
    return o + off, o + off, R.normalize(d + eps * u), R.normalize(d + eps * v)


def random_rows(geo, seed, n, on_surface=0.2):
    """rays aimed into each primitive's bounding ball (1.25 x: about a third miss) from outside, inside and (a share `on_surface`) on the surface;
    t_max infinite, 0.2 % (of the distance or the primitive's size) above or below the binary64 hit distance (the binary32 neighbours of t are in the edge table), or anywhere; differentials of 1e-3 .. 1e-1 radians or none; wi anywhere; the three etas"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(geo), n)
    c = np.array([g.centre for g in geo])[k]
    rad = np.array([g.radius for g in geo])[k][:, None]
    ball = lambda: unit(rng, n) * np.cbrt(rng.uniform(0.0, 1.0, (n, 1)))
    target = c + 1.25 * rad * ball()
    where = rng.choice(3, n, p=[0.8 - on_surface, 0.2, on_surface])
    on = np.zeros((n, 3))
    for i, g in enumerate(geo):
        on[k == i] = g.surface(rng, int(np.sum(k == i)))
    o = np.where((where == 0)[:, None], c + rad * rng.uniform(1.5, 6.0, (n, 1)) * unit(rng, n), np.where((where == 1)[:, None], c + 0.8 * rad * ball(), on))
    o = o.astype(f32).astype(np.float64)
    d = R.normalize(target - o).astype(f32).astype(np.float64)
    t = np.zeros(n)
    for i, g in enumerate(geo):
        t[k == i] = g.t_of(o[k == i], d[k == i])
    t = np.where(np.isfinite(t) & (t > 0.0), t, 1.0)
    how = rng.choice(4, n, p=[0.7, 0.1, 0.1, 0.1])
    t_max = np.select([how == 0, how == 1, how == 2], [np.inf, t + 2.0e-3 * np.maximum(t, rad[:, 0]), t - 2.0e-3 * np.maximum(t, rad[:, 0])], t * rng.uniform(0.0, 2.0, n))
    has = (rng.uniform(size=n) < 0.85).astype(f32)
    lens = np.where(rng.uniform(size=(n, 1)) < 0.3, 0.01 * rad, 0.0)
    rxo, ryo, rxd, ryd = differential(o, d, 10.0 ** rng.uniform(-3.0, -1.0, n), lens, rng)
    return make_rows(o, d, k, t_max, rng.uniform(0.0, 1.0, n), has, rxo, ryo, rxd, ryd, unit(rng, n), rng.choice([1.5, 1.0 / 1.5, 1.0], n), (rng.uniform(size=n) < 0.5).astype(f32))


def hitting_rows(geo, seed, n, eps=1.0e-2, has=1.0, lens=0.0, inside=0.0):
    """rays from outside that hit well inside each primitive (a triangle's barycentrics all above 0.05, a sphere away from its limb), at an incidence
    of at most about 70 degrees (a share `inside` of a sphere's rays start inside it instead); t_max infinite; differentials of `eps` radians"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(geo), n)
    target, normal = np.zeros((n, 3)), np.zeros((n, 3))
    for i, g in enumerate(geo):
        m = int(np.sum(k == i))
        if g.kind == "tri":
            b = 0.05 + 0.85 * rng.dirichlet((1.0, 1.0, 1.0), m)
            target[k == i], normal[k == i] = b @ g.p, g.ng
        else:
            s = unit(rng, m)
            target[k == i] = R.tf_point(g.o2w, g.r * s)
            normal[k == i] = R.normalize(R.tf_normal(g.o2w_inv, s))
    rad = np.array([g.radius for g in geo])[k][:, None]
    side = np.where(rng.uniform(size=(n, 1)) < 0.5, 1.0, -1.0) * np.array([1.0 if g.kind == "tri" else 0.0 for g in geo])[k][:, None] + np.array([0.0 if g.kind == "tri" else 1.0 for g in geo])[k][:, None]
    away = R.normalize(side * normal + 0.9 * rng.uniform(0.0, 1.0, (n, 1)) * unit(rng, n))
    o = target + away * rad * rng.uniform(1.5, 4.0, (n, 1))
    within = rng.uniform(size=n) < inside              # spheres: from inside, so that the ray leaves the medium
    for i, g in enumerate(geo):
        m = within & (k == i) & (g.kind == "sph")
        o[m] = R.tf_point(g.o2w, 0.5 * g.r * unit(rng, int(m.sum()))) if g.kind == "sph" else o[m]
    o = o.astype(f32).astype(np.float64)
    d = R.normalize(target - o).astype(f32).astype(np.float64)
    rxo, ryo, rxd, ryd = differential(o, d, eps, lens * rad, rng if lens else None)
    return make_rows(o, d, k, np.inf, rng.uniform(0.0, 1.0, n), has, rxo, ryo, rxd, ryd, unit(rng, n), 1.5, 1.0)


# ---------------------------------------------------------------- layer 2: properties no reading of the reference enters
def dot3(a, b): return np.sum(a * b, axis=1)
def norm3(a): return np.sqrt(dot3(a, a))


def check_primitive_mapping(hook):
    """a ray aimed at each builder primitive's centroid hits exactly one BVH index through the hook, and that index is where the library's order puts
    the primitive: the order is a bijection"""
    geo, n = hook.geo, len(hook.geo)
    assert sorted(hook.order.tolist()) == list(range(n))
    for i, g in enumerate(geo):
        aim = g.centre if g.kind == "tri" else R.tf_point(g.o2w, g.r * R.normalize(np.array([0.3, 0.4, 0.1])))
        o = aim + (g.ng if g.kind == "tri" else R.normalize(aim - g.centre)) * g.radius * 2.0
        hits = hook.raw(make_rows(o, R.normalize(aim - o), np.arange(n)), bvh_indices=True)[:, 0] != 0.0
        assert hits.sum() == 1 and hook.order[int(np.argmax(hits))] == i, (hook.name, i, hits)


def check_error_box(hook, n=100000, seed=71):
    """triangle: |p - sum b_i p_i| <= p_err per component, in binary64 with the returned barycentrics.  Sphere: the distance of p from the sphere in
    object space is at most |W| |p_err| (W the linear part of world-to-object, |W| its largest singular value: a world-space displacement e inside the
    box moves the object-space point by W e), plus what the binary32 inverse in W itself is off by: 8 ulps of the object-space point's size"""
    rows = random_rows(hook.targets, seed, n)
    o = hook(rows)
    k, hit = prim_of(rows), o["hit"]
    assert hit.sum() > n // 20
    for i, g in enumerate(hook.targets):
        m = hit & (k == i)
        if g.kind == "tri":
            exact = o["bary"][m] @ g.p
            bad = np.abs(o["p"][m] - exact) > o["p_err"][m]
            assert not bad.any(), (hook.name, int(bad.any(axis=1).sum()), int(m.sum()))
        else:
            po = R.tf_point(g.w2o, o["p"][m])
            dist = np.abs(norm3(po) - g.r)
            bound = np.linalg.norm(g.w2o[:3, :3], 2) * norm3(o["p_err"][m]) + 8.0 * EPS * (norm3(po) + norm3(R.tf_vector(g.w2o, o["p"][m])) + np.linalg.norm(g.w2o[:3, 3]))
            assert np.all(dist <= bound), (hook.name, float(np.max(dist / bound)))


def spawn_rows(hook, n, seed):
    """hits, each bounced along a wi on either side of the surface -> (rows, their output, rows of the spawned rays aimed back at the same primitive)"""
    rows = hitting_rows(hook.targets, seed, n)
    o = hook(rows)
    again = make_rows(o["spawn_o"], rows[:, 22:25].astype(np.float64), prim_of(rows))
    return rows, o, again


def check_spawned_ray_leaves(hook, n=50000, seed=72):
    """the origin of spawn_ray(hit, wi) lies on wi's side of the plane through p with normal n, by at least dot(|n|, p_err) (x (1 - 1e-6): n is unit to
    within a few binary32 ulps, and each component of the origin is rounded AWAY from the plane); fed back, the ray misses a triangle and does not hit a
    sphere closer than its far side (half the chord along wi; rays within 1e-3 of grazing are left out: their far side is as close as the offset).
    A sphere's re-hit is only claimed where wi is on the same side of the returned n as of the surface's own normal (the transposed inverse applied to
    the object-space point): under a rotation and a non-uniform scale the reference's transform_normal gives another n, and a wi
    between the two starts outside and enters, or the reverse.  -> the share of a sphere's rows where the two normals disagree about wi"""
    rows, o, again = spawn_rows(hook, n, seed)
    hit = o["hit"]
    assert hit.mean() > 0.3
    wi = rows[:, 22:25].astype(np.float64)
    side = np.sign(dot3(wi, o["n"]))
    moved = dot3(o["spawn_o"] - o["p"], o["n"]) * side
    need = dot3(np.abs(o["n"]), o["p_err"])
    assert np.all(moved[hit] >= need[hit] * (1.0 - 1.0e-6)), (hook.name, float(np.min(moved[hit] / need[hit])))
    assert np.all(o["spawn_tmax"][hit] == np.inf)
    back = hook(again)
    k = prim_of(rows)
    disagree = 0.0
    for i, g in enumerate(hook.targets):
        m = hit & (k == i)
        if g.kind == "tri":
            assert not back["hit"][m].any(), (hook.name, "spawned rays that hit their own triangle", float(np.mean(back["hit"][m])))
        else:
            po, dd = R.tf_point(g.w2o, o["p"][m]), R.tf_vector(g.w2o, wi[m])
            true_n = R.normalize(po @ g.w2o[:3, :3])
            true_n = true_n * np.sign(dot3(true_n, o["n"][m]))[:, None]
            agree = np.sign(dot3(wi[m], true_n)) == side[m]
            disagree = float(np.mean(~agree))
            far = -2.0 * dot3(po, dd) / dot3(dd, dd)
            cosine = dot3(po, dd) / (norm3(po) * norm3(dd))
            bh, bt = back["hit"][m], back["t"][m]
            ok = (np.abs(cosine) < 1.0e-3) | ~agree | ~bh | ((far > 0.0) & (bt >= 0.5 * far))
            assert ok.all(), (hook.name, "spawned rays that hit their own sphere on the near side", int((~ok).sum()))
    return disagree


def check_frames(hook, n=100000, seed=73):
    rows = random_rows(hook.targets, seed, n)
    o = hook(rows)
    k, hit = prim_of(rows), o["hit"]
    raw_in, out = rows, hook.raw(rows)
    assert np.all(out[hit, 14] == raw_in[hit, 7]), "time is passed through"
    unit_tol = 8.0 * EPS                             # a normalised binary32 vector: three squares, two sums, a root and three divisions
    assert np.all(np.abs(norm3(o["n"][hit]) - 1.0) <= unit_tol) and np.all(np.abs(norm3(o["ns"][hit]) - 1.0) <= unit_tol)
    for i, g in enumerate(hook.targets):
        m = hit & (k == i)
        if g.kind == "tri":
            assert same_bits_or_both_nan(out[m, 15:18], -raw_in[m, 3:6]).all(), "wo = -d, exactly"
            # n is the normalised cross product of two edges whose coordinates carry half an ulp of the vertices' size each
            tol = 16.0 * EPS * max(1.0, float(np.max(np.abs(g.p))) / float(np.min(np.linalg.norm(g.p - np.roll(g.p, 1, axis=0), axis=1))))
            for e in (g.p[1] - g.p[0], g.p[2] - g.p[1], g.p[0] - g.p[2]):
                assert np.all(np.abs(o["n"][m] @ R.normalize(e)) <= tol), (hook.name, "n is not perpendicular to an edge")
            if g.n is not None or g.s is not None:
                assert np.all(dot3(o["n"][m], o["ns"][m]) >= -unit_tol), (hook.name, "n and ns on opposite sides")
                assert np.all(np.abs(norm3(o["s_dpdu"][m]) - 1.0) <= 2.0 * unit_tol), (hook.name, "shading dpdu is not unit")
                assert np.all(np.abs(dot3(o["s_dpdu"][m], o["ns"][m])) <= 2.0 * unit_tol), (hook.name, "shading dpdu is not perpendicular to ns")
            else:
                assert same_bits_or_both_nan(out[m, 11:14], out[m, 18:21]).all(), "no shading frame: ns = n"
        else:
            d = raw_in[m, 3:6].astype(np.float64)
            want = R.normalize(R.tf_vector(g.o2w, -R.tf_vector(g.w2o, d)))
            assert np.all(np.abs(o["wo"][m] - want) <= 1.0e-5), (hook.name, "wo")
            assert np.all(dot3(o["n"][m], o["ns"][m]) >= 1.0 - unit_tol)


def check_derivatives(hook, n=40000, seed=74):
    """triangles with non-degenerate uvs: p_A - p_B = dpdu du + dpdv dv for pairs of hits on one triangle, in binary64 from the returned p and uv (the
    barycentrics are good to a few ulps, so uv is off by that share of its size and p by dpdu, dpdv times that).  Spheres under a translation: uv gives
    p back through the parametrisation, dpdu / dpdv are its derivatives (central differences), dndu = +-dpdu / r, dndv = +-dpdv / r"""
    rows = hitting_rows(hook.targets, seed, n)
    o = hook(rows)
    k, hit = prim_of(rows), o["hit"]
    for i, g in enumerate(hook.targets):
        m = np.flatnonzero(hit & (k == i))
        if g.kind == "tri":
            if g.degenerate_uv:
                continue
            a, b = m[: len(m) // 2 * 2: 2], m[1: len(m) // 2 * 2: 2]
            duv = o["uv"][a] - o["uv"][b]
            resid = (o["p"][a] - o["p"][b]) - (o["dpdu"][a] * duv[:, 0:1] + o["dpdv"][a] * duv[:, 1:2])
            size = float(np.max(np.abs(g.p))) + (norm3(o["dpdu"][a]) + norm3(o["dpdv"][a])) * max(1.0, float(np.max(np.abs(g.uv))))
            assert np.all(np.abs(resid).max(axis=1) <= 64.0 * EPS * size), (hook.name, float(np.max(np.abs(resid).max(axis=1) / size)) / EPS)
            assert same_bits_or_both_nan(hook.raw(rows)[a, 28:34], hook.raw(rows)[b, 28:34]).all(), "dpdu and dpdv are constants of the triangle"
        elif hook.name in TRANSLATED_SPHERES:
            def param(u, v):
                phi, th = u * g.phi_max, g.theta_min + v * (g.theta_max - g.theta_min)
                return g.centre + g.r * np.stack([np.sin(th) * np.cos(phi), np.sin(th) * np.sin(phi), np.cos(th)], axis=1)
            u, v = o["uv"][m, 0], o["uv"][m, 1]
            th = g.theta_min + v * (g.theta_max - g.theta_min)
            m2 = np.abs(np.sin(th)) > 1.0e-2          # acos loses the angle next to the poles
            size = np.abs(g.centre).max() + g.r
            assert np.all(np.abs(param(u, v) - o["p"][m])[m2] <= 64.0 * EPS * size / 1.0e-2), (hook.name, "uv does not give p back")
            h = 1.0e-6
            du, dv = (param(u + h, v) - param(u - h, v)) / (2.0 * h), (param(u, v + h) - param(u, v - h)) / (2.0 * h)
            for got, want in ((o["dpdu"][m], du), (o["dpdv"][m], dv)):
                assert np.all(np.abs(got - want)[m2] <= 1.0e-4 * (norm3(want)[m2, None] + g.r)), (hook.name, "dpdu / dpdv are not the derivatives")
            for got, want in ((o["dndu"][m], o["dpdu"][m] / g.r), (o["dndv"][m], o["dpdv"][m] / g.r)):
                e = np.minimum(np.abs(got - want).max(axis=1), np.abs(got + want).max(axis=1))
                assert np.all(e[m2] <= 1.0e-4 * (norm3(want)[m2] + 1.0)), (hook.name, "dndu / dndv are not dpdu / r, dpdv / r", float(np.max(e[m2])))


def tex_system_determinant(o):
    """the 2 x 2 system of compute_tex_differentials in binary64 from the returned n, dpdu, dpdv -> (determinant, the two coordinates, whether the
    choice of coordinates is a near tie)"""
    an = np.abs(o["n"])
    first = (an[:, 0] > an[:, 1]) & (an[:, 0] > an[:, 2])
    second = ~first & (an[:, 1] > an[:, 2])
    d0 = np.where(first, 1, 0)
    d1 = np.where(first | second, 2, 1)
    r = np.arange(len(an))
    det = o["dpdu"][r, d0] * o["dpdv"][r, d1] - o["dpdv"][r, d0] * o["dpdu"][r, d1]
    return det, d0, d1


def check_texture_differentials(hook, n=40000, seed=75):
    """dpdx lies in the tangent plane, p + dpdx lies on the auxiliary ray, dpdx = dudx dpdu + dvdx dpdv (and y); all zero without a differential or
    with a singular system (|determinant| < 1e-10: the sliver).  The bound: the plane intersection cancels |p|-sized terms and divides by n . rxd
    (rows steeper than 0.1 only), then adds a |t|-sized product.  Under a rotation and a non-uniform scale n is not perpendicular to dpdu, dpdv
    (DESIGN.md 3.2): there only the two coordinates the system was solved in are compared"""
    rows = hitting_rows(hook.targets, seed, n, eps=3.0e-2, lens=0.01)
    rows[::5, 9] = 0.0
    o = hook(rows)
    hit = o["hit"]
    det, d0, d1 = tex_system_determinant(o)
    singular, regular = np.abs(det) < 1.0e-10 * (1.0 - 1.0e-3), np.abs(det) > 1.0e-10 * (1.0 + 1.0e-3)
    none = hit & ((rows[:, 9] == 0.0) | singular)
    assert none.sum() > 0
    for c in ("dpdx", "dpdy", "dudx", "dvdx", "dudy", "dvdy"):
        assert np.all(o[c][none] == 0.0), (hook.name, c, "is not zero without a differential or with a singular system")
    for c in ("rxo", "ryo", "rxd", "ryd"):
        assert np.all(o[c][hit & (rows[:, 9] == 0.0)] == 0.0), (hook.name, c, "is not zero without a differential")
    r = np.arange(n)
    for x, (dp, du, dv) in dict(x=("dpdx", "dudx", "dvdx"), y=("dpdy", "dudy", "dvdy")).items():
        ro, rdir = (rows[:, 10:13], rows[:, 16:19]) if x == "x" else (rows[:, 13:16], rows[:, 19:22])
        ro, rdir = ro.astype(np.float64), rdir.astype(np.float64)
        steep = np.abs(dot3(o["n"], rdir))
        m = hit & (rows[:, 9] != 0.0) & (steep > 0.1) & regular
        if singular[hit].all():
            continue
        assert m.sum() > 0.3 * n, (hook.name, int(m.sum()))
        assert np.all((o[du] != 0.0) | (o[dv] != 0.0) | (norm3(o[dp]) == 0.0))
        size = (np.abs(o["p"]).max(axis=1) + np.abs(ro).max(axis=1) + norm3(o["p"] - ro)) / np.maximum(steep, 0.1)
        tol = 64.0 * EPS * size
        assert np.all(np.abs(dot3(o["n"], o[dp]))[m] <= tol[m] + 8.0 * EPS * norm3(o[dp])[m]), (hook.name, dp, "leaves the tangent plane")
        q = o["p"] + o[dp] - ro
        off = norm3(q - rdir * (dot3(q, rdir) / dot3(rdir, rdir))[:, None])
        assert np.all(off[m] <= tol[m]), (hook.name, "p + " + dp + " is off the auxiliary ray", float(np.max(off[m] / tol[m])))
        resid = np.abs(o[dp] - (o["dpdu"] * o[du][:, None] + o["dpdv"] * o[dv][:, None]))
        solved = np.maximum(resid[r, d0], resid[r, d1])
        # the solve divides by the determinant: its rounding is that of the products |dpdu| |dpdv| against the determinant itself
        cond = norm3(o["dpdu"]) * norm3(o["dpdv"]) / np.maximum(np.abs(det), 1.0e-300)
        bound = 16.0 * (tol + EPS * norm3(o[dp])) * cond
        assert np.all(solved[m] <= bound[m]), (hook.name, dp, "is not dudx dpdu + dvdx dpdv", float(np.max(solved[m] / bound[m])))
        if hook.name != "sph_scaled":
            # the third coordinate follows as far as dpdx lies in the plane of dpdu, dpdv: on a sphere it leaves that plane by |dpdx|^2 / r
            bend = 0.0 if hook.targets[0].kind == "tri" else norm3(o[dp]) ** 2 / hook.targets[0].r
            assert np.all(resid.max(axis=1)[m] <= 4.0 * bound[m] + 2.0 * bend[m] if np.ndim(bend) else resid.max(axis=1)[m] <= 4.0 * bound[m]), (hook.name, dp, "third coordinate")


def reflect_about(w, n):
    """-w + 2 (w . n) n, n as given (not normalised: what the first-order formula expands)"""
    return -w + 2.0 * dot3(w, n)[:, None] * n


def refract_through(w, n, eta):
    """reflection/mod.rs:75-83 in binary64: w and n on the same side, eta = eta_i / eta_t -> (transmitted direction, total internal reflection)"""
    ci = dot3(n, w)
    s2t = eta * eta * np.maximum(0.0, 1.0 - ci * ci)
    ct = np.sqrt(np.maximum(1.0 - s2t, 0.0))
    return -eta[:, None] * w + (eta * ci - ct)[:, None] * n, s2t >= 1.0


def bounce_residual(hook, eps, reflect, seed, n, eta=1.5):
    """the returned rx / ry directions of a specular bounce against the exact bounce of the auxiliary ray about the surface's own normal there,
    ns + dndx -> (|residual| as returned, |residual| with the named correction added, rows that count, side: +1 entering (wo . ns > 0), -1 leaving).
    The corrections are the two places where the reference's expansion is not the derivative of the bounce:
      reflect   the reference adds dDN ns where the derivative of 2 (wo . n) n has 2 dDN ns (integrator/mod.rs:74-75): correction + dDN ns;
      transmit  d mu = (eta - eta^2 cos_i / cos_t) dDN with cos_t = |wi . n|; the reference divides by wi . n, which is negative (:146-153), and takes
                dDN from the unflipped normal when the ray leaves (:141-142): correction (c_true dDN_true - c_ref dDN_ref) n."""
    rows = hitting_rows(hook.targets, seed, n, eps=eps, inside=0.5)
    first = hook(rows)
    wo, ns = first["wo"], first["ns"]
    etas = np.full(n, eta)
    side = np.where(dot3(wo, ns) > 0.0, 1.0, -1.0)
    sn = ns * side[:, None]
    rel = np.where(side > 0.0, 1.0 / etas, etas)
    if reflect:
        wi, tir = reflect_about(wo, ns), np.zeros(n, bool)
    else:
        wi, tir = refract_through(wo, sn, rel)
    rows[:, 22:25], rows[:, 25], rows[:, 26] = wi, eta, 1.0 if reflect else 0.0
    o = hook(rows)
    wi = rows[:, 22:25].astype(np.float64)
    use = o["hit"] & ((o["dudx"] != 0.0) | (o["dvdx"] != 0.0)) & ~tir & np.isfinite(wi).all(axis=1)
    plain, fixed = [], []
    for aux, du, dv, got in ((rows[:, 16:19], "dudx", "dvdx", "rxd"), (rows[:, 19:22], "dudy", "dvdy", "ryd")):
        dndx = o["dndu"] * o[du][:, None] + o["dndv"] * o[dv][:, None]
        wx = -aux.astype(np.float64)
        dwo = wx - wo
        if reflect:
            exact = reflect_about(wx, ns + dndx)
            corr = (dot3(dwo, ns) + dot3(wo, dndx))[:, None] * ns
        else:
            exact, t2 = refract_through(wx, R.normalize(sn + dndx * side[:, None]), rel)
            use &= ~t2
            ci, ct = dot3(wo, sn), np.abs(dot3(wi, sn))
            d_true, d_ref = dot3(dwo, sn) + dot3(wo, dndx * side[:, None]), dot3(dwo, ns) + dot3(wo, dndx * side[:, None])
            with np.errstate(all="ignore"):
                corr = ((rel - rel * rel * ci / ct) * d_true - (rel + rel * rel * ci / ct) * d_ref)[:, None] * sn
        with np.errstate(all="ignore"):
            plain.append(norm3(o[got] - exact))
            fixed.append(norm3(o[got] + corr - exact))
    return np.maximum(*plain), np.maximum(*fixed), use, side


# the bounced differential is meant to be the first-order expansion of the exact bounce in the auxiliary ray's offset: what is left is second order, so
# halving the offset quarters it.  Asserted: the median residual at eps / 2 is at most 0.35 x the one at eps (a first-order error gives 0.5, a
# second-order one 0.25; 0.35 leaves the third-order term at eps = 2e-2 room), or both are at binary32 rounding (flat surfaces, exact expansion)
BOUNCE_EPS, BOUNCE_FALL, BOUNCE_ROUNDING = 2.0e-2, 0.35, 64.0 * EPS


def bounce_fall(hook, reflect, side=None, seed=76, n=20000):
    """-> medians of (residual at eps, at eps / 2, corrected residual at eps, at eps / 2)"""
    a, ca, use_a, s = bounce_residual(hook, BOUNCE_EPS, reflect, seed, n)
    b, cb, use_b, _ = bounce_residual(hook, BOUNCE_EPS / 2.0, reflect, seed, n)
    m = use_a & use_b & (True if side is None else s == side)
    if m.sum() < n // 50:
        return None
    return tuple(float(np.median(x[m])) for x in (a, b, ca, cb))


def check_bounced_differential(hook, reflect, side):
    """with the named correction the returned differential is the neighbouring ray to second order; as returned it is not (the quirk, pinned: the
    residual only halves) wherever the missing term is not itself zero"""
    r = bounce_fall(hook, reflect, side)
    assert r is not None, (hook.name, reflect, side, "too few rows with a solved differential on this side")
    a, b, ca, cb = r
    assert cb <= max(BOUNCE_FALL * ca, BOUNCE_ROUNDING), (hook.name, reflect, side, r)
    assert ca <= 100.0 * BOUNCE_EPS ** 2, (hook.name, reflect, side, r)       # second order at all: a few curvatures (|dndu| <= 5 here) times eps^2
    if a > 16.0 * ca:                                 # the quirk shows: first order, the residual halves
        assert 0.45 * a <= b <= 0.55 * a, (hook.name, reflect, side, r)
    return r


def check_sanity(hook, n=100000, seed=77):
    """every output is finite on finite inputs (spawn_ray's t_max is the one infinity)"""
    out = hook.raw(random_rows(hook.targets, seed, n))
    fin = np.isfinite(out)
    fin[:, 53] |= out[:, 53] == np.inf
    fin[:, 24:26] = True
    assert fin.all(), (hook.name, np.argwhere(~fin)[:5].tolist())
    assert 0.05 < np.mean(out[:, 0] != 0.0) < 0.95, (hook.name, float(np.mean(out[:, 0] != 0.0)))


def check_refusals(be):
    """null pointers, a primitive index outside the scene (below 0, n_prims, far beyond, the bits of a float); n == 0 is a no-op"""
    h = Hook(be, "tri_pair")
    rows = random_rows(h.geo, 3, 8)
    out = np.full((8, NOUT), 7.0, f32)
    pr, po = rows.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    bad = [(None, pr, 8, po), (h.scene.handle, None, 8, po), (h.scene.handle, pr, 8, None)]
    codes = [h.fn(*a) for a in bad]
    for value in (-1, 2, 1 << 30, int(np.array([1.0], f32).view(np.int32)[0])):
        r2 = rows.copy(); r2[5:6, 8:9].view(np.int32)[0, 0] = value
        codes.append(h.fn(h.scene.handle, r2.ctypes.data_as(C.c_void_p), 8, po))
    assert all(rc == A.FTN_ERR_INVALID_ARGUMENT for rc in codes), codes
    assert np.all(out == 7.0)
    assert h.fn(h.scene.handle, pr, 0, po) == A.FTN_OK and np.all(out == 7.0)
    assert h.fn(h.scene.handle, pr, 8, po) == A.FTN_OK and not np.any(out == 7.0)
    return codes


# ---------------------------------------------------------------- the edge table
def edge_rays(g):
    """(o, d) through each vertex and along each edge, in the plane, from the plane, 1e-30 and 3e20 off it; d with a zero component, tiny, not unit;
    a sphere's poles, seam, clipping planes, limb and centre"""
    rays = []
    if g.kind == "tri":
        p0, p1, p2 = g.p
        c, n, r = g.centre, g.ng, g.radius
        eye = c + n * 2.0 * r + (p1 - p0) * 0.3
        targets = [p0, p1, p2, 0.5 * (p0 + p1), 0.5 * (p1 + p2), 0.5 * (p2 + p0), 0.25 * p0 + 0.75 * p1, c]
        for t in targets:
            rays.append((eye, R.normalize(t - eye)))
            rays.append((t + np.array([0.0, 0.0, 2.0 * r]), np.array([0.0, 0.0, -1.0])))           # axis-aligned: d has two zero components
            rays.append((t + np.array([0.0, 2.0 * r, 2.0 * r]), np.array([0.0, -1.0, -1.0])))      # one zero component, not unit
        rays += [(p0 - (p1 - p0), R.normalize(p1 - p0)), (c - (p1 - p0) * 3.0, R.normalize(p1 - p0)),      # along an edge, in the plane
                 (c, n), (c, -n), (c + n * 1.0e-30, -n), (c + n * 1.0e-30, n), (c + n * 1.0e-6 * r, -n),    # from the plane and next to it
                 (c + n * 3.0e20, -n), (c - n * 3.0e20, n),                                                  # 3e20 off it: the edge functions overflow
                 (eye, R.normalize(c - eye) * 1.0e-20), (eye, R.normalize(c - eye) * 37.5), (eye, R.normalize(c - eye) * 3.0e20), (eye, np.zeros(3)),
                 (eye, R.normalize(eye - c))]
    else:
        r = g.r
        w = lambda v: R.tf_point(g.o2w, np.asarray(v, np.float64))
        wv = lambda v: R.tf_vector(g.o2w, np.asarray(v, np.float64))
        far = 3.0 * r
        zc = [g.z_min, g.z_max, 0.5 * (g.z_min + g.z_max)]
        for z in zc:                                      # through the clipping planes and between them, from four sides
            rr = np.sqrt(max(r * r - z * z, 0.0))
            for ph in (0.0, 1.0e-7, 0.5 * g.phi_max, g.phi_max, g.phi_max + 1.0e-4, 2.0 * np.pi - 1.0e-7):
                q = np.array([rr * np.cos(ph), rr * np.sin(ph), z])
                rays.append((w(q * 3.0 + np.array([0.0, 0.0, 0.1 * r])), R.normalize(w(q) - w(q * 3.0 + np.array([0.0, 0.0, 0.1 * r])))))
        rays += [(w([0, 0, far]), wv([0, 0, -1.0])), (w([0, 0, -far]), wv([0, 0, 1.0])), (w([0, 0, 0]), wv([0, 0, 1.0])), (w([0, 0, 0]), wv([0, 0, -1.0])),     # the poles
                 (w([0, 0, 0]), wv([1.0, 0, 0])), (w([0, 0, 0]), wv([0.3, -0.5, 0.4])), (w([0, 0, 0]), np.zeros(3)),                                            # from the centre
                 (w([far, 0, 0]), wv([-1.0, 0, 0])), (w([far, -1.0e-7 * r, 0]), wv([-1.0, 0, 0])), (w([-far, 0, 0]), wv([1.0, 0, 0])),                           # the seam
                 (w([r, -far, 0]), wv([0, 1.0, 0])), (w([r * (1.0 - 1.0e-7), -far, 0]), wv([0, 1.0, 0])), (w([r * (1.0 + 1.0e-6), -far, 0]), wv([0, 1.0, 0])), # the limb
                 (w([r, 0, 0]), wv([1.0, 0, 0])), (w([r, 0, 0]), wv([-1.0, 0, 0])), (w([0.6 * r, 0, 0.8 * r]), wv([0, 1.0, 0])),                                 # from the surface
                 (w([far, 0.2 * r, 0.3 * r]), wv([-1.0e-20, 0, 0])), (w([far, 0.2 * r, 0.3 * r]), wv([-37.5, 0, 0])), (w([far, 0.2 * r, 0.3 * r]), wv([-3.0e20, 0, 0]))]
    return rays


def edge_rows(geo):
    """every ray of edge_rays() with t_max infinite and at the binary64 hit distance and its binary32 neighbours (three ulps each way), and, for a few,
    differentials along the surface, zero, tiny and overflowing, wi in the surface, +-n, zero, eta 1, grazing wo"""
    rows = []
    for i, g in enumerate(geo):
        rays = edge_rays(g)
        o, d = np.array([r[0] for r in rays]), np.array([r[1] for r in rays])
        o32, d32 = o.astype(f32).astype(np.float64), d.astype(f32).astype(np.float64)
        with np.errstate(all="ignore"):
            t = np.nan_to_num(g.t_of(o32, d32), nan=1.0, posinf=1.0, neginf=1.0).astype(f32)
        tm = [np.full(len(o), np.inf, f32), t]
        lo, hi = t, t
        for _ in range(3):
            lo, hi = below(lo), above(hi)
            tm += [lo, hi]
        normal = g.ng if g.kind == "tri" else R.normalize(np.array([0.3, 0.2, 0.9]))
        tangent = R.normalize(np.cross(normal, [0.3, -0.7, 0.2]))
        rxo, ryo, rxd, ryd = differential(o32, np.where(norm3(d32)[:, None] > 0.0, d32, [0.0, 0.0, 1.0]), 1.0e-2)
        for t_max in tm:
            rows.append(make_rows(o, d, i, t_max, 0.25, 1.0, rxo, ryo, rxd, ryd, wi=normal + tangent, eta=1.5, reflect=1.0))
        few = slice(0, len(o), 3)
        n_few = len(o[few])
        for wi in (tangent, normal, -normal, np.zeros(3), tangent * 1.0e-20, normal * 3.0e20):
            for eta, refl in ((1.0, 0.0), (1.5, 0.0), (1.0 / 1.5, 0.0), (1.0, 1.0)):
                rows.append(make_rows(o[few], d[few], i, np.inf, 0.5, 1.0, rxo[few], ryo[few], rxd[few], ryd[few], wi=wi, eta=eta, reflect=refl))
        for axd in (tangent, np.zeros(3), tangent * 1.0e-30, tangent * 3.0e20, -d32[few]):             # along the surface: dot(n, rxd) = 0 on a triangle
            for axo in (o[few], o[few] + tangent * 1.0e-30, o[few] + 3.0e20):
                rows.append(make_rows(o[few], d[few], i, np.inf, 0.5, 1.0, axo, axo, np.broadcast_to(axd, (n_few, 3)), np.broadcast_to(axd, (n_few, 3)), wi=normal, eta=1.5, reflect=0.0))
        if g.kind == "tri":                               # grazing wo: from inside the triangle's plane, lifted by a few ulps
            for lift in (1.0e-7, 1.0e-5, 1.0e-3):
                eye = g.centre + (g.p[1] - g.p[0]) * 4.0 + g.ng * lift * g.radius
                rows.append(make_rows(eye, R.normalize(g.centre - eye), i, np.inf, 0.5, 1.0, eye, eye, *differential(eye[None], R.normalize(g.centre - eye)[None], 1.0e-3)[2:], wi=normal, eta=1.5, reflect=1.0))
    return np.concatenate(rows)


def undefined_by_the_reference(geo, rows):
    """-> rows whose outcome the reference's text leaves to the implementation: on a TRIANGLE a ray whose origin or direction reaches 1e18 makes the
    edge functions overflow to inf - inf = NaN, a zero direction makes them 0 / 0 = NaN, and sign_differs (triangle.rs:428-434) then goes by the
    NaN's sign bit.  Only the ray itself counts: an overflowing differential or wi yields NaNs that both sides must agree on.  A
    sphere's test has no such step (a NaN fails every comparison of sphere.rs:92-110 the same way everywhere): its rows are never exempt."""
    r = rows.astype(np.float64)
    tri = np.array([g.kind == "tri" for g in geo])[prim_of(np.ascontiguousarray(rows))]
    with np.errstate(all="ignore"):
        return tri & (~np.isfinite(r[:, 0:6]).all(axis=1) | (np.abs(r[:, 0:6]).max(axis=1) > 1.0e18) | ~(np.abs(r[:, 3:6]).max(axis=1) > 0.0))


# ---------------------------------------------------------------- cameras
def cameras(be):
    """name -> (PerspectiveCamera, thin lens?, (shutter open, close), orthonormal camera-to-world?)"""
    ident = Transform.identity(be)
    look = (Transform.identity(be) * Transform.look_at(be, (1.0, 2.0, 3.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0))).inverse()
    far = Transform.translate(be, (10000.0, -10000.0, 10000.0)) * Transform.rotate(be, 37.0, (1.0, 2.0, 3.0))
    return {
        "pinhole": (PerspectiveCamera(be, look, (64, 64), fov=60.0), False, (0.0, 1.0), True),
        "thin_lens": (PerspectiveCamera(be, look, (64, 64), fov=60.0, lens_radius=0.05, focal_dist=3.0), True, (0.0, 1.0), True),
        "wide": (PerspectiveCamera(be, look, (80, 56), fov=45.0), False, (0.0, 1.0), True),
        "window": (PerspectiveCamera(be, look, (64, 48), screen_window=(-0.2, 0.1, 1.4, 0.9), fov=50.0, lens_radius=0.02, focal_dist=5.0), True, (0.0, 1.0), True),
        "shutter": (PerspectiveCamera(be, ident, (32, 32), shutter=(0.25, 1.75), fov=90.0), False, (0.25, 1.75), True),
        "far_rotated": (PerspectiveCamera(be, far, (64, 64), fov=60.0, lens_radius=0.1, focal_dist=8.0), True, (0.0, 1.0), True),
    }


CAMERA_NAMES = ["pinhole", "thin_lens", "wide", "window", "shutter", "far_rotated"]
CAMERA_RES = dict(pinhole=(64, 64), thin_lens=(64, 64), wide=(80, 56), window=(64, 48), shutter=(32, 32), far_rotated=(64, 64))
SPPS = [1, 4, 16]


def camera_raw(be, cam, spp, rows):
    assert cam.be is be
    return cam.test_rays(spp, rows)


def camera_rows(name, seed, n):
    rng = np.random.default_rng(seed)
    w, h = CAMERA_RES[name]
    rows = np.zeros((n, CIN), f32)
    rows[:, 0], rows[:, 1] = rng.uniform(0.0, w, n), rng.uniform(0.0, h, n)
    rows[:, 2:5] = rng.uniform(0.0, 1.0, (n, 3))
    return rows


def camera_edge_rows(name):
    w, h = CAMERA_RES[name]
    films = [(0, 0), (w, 0), (0, h), (w, h), (w / 2, h / 2), (-3, -5), (w + 7.5, h + 0.25), (0.5, 0.5), (below(w), below(h))]
    one = below(1.0)
    lenses = [(0, 0), (0.5, 0.5), (one, one), (0, one), (one, 0), (0.25, 0.25), (0.25, 0.75), (0.75, 0.25), (0.5, 0.25), (0.25, 0.5), (0.5, above(0.5)), (above(0.5), 0.5), (0.1, 0.9)]
    return np.array([(a, b, c, d, t, 0, 0, 0) for a, b in films for c, d in lenses for t in (0.0, 1.0, 0.5)], f32)


def check_camera(be, name):
    cam, lens, (t0, t1), ortho = cameras(be)[name]
    rows = camera_rows(name, 81, 20000)
    outs = {spp: camera_raw(be, cam, spp, rows).astype(np.float64) for spp in SPPS}
    o = outs[1]
    assert np.isfinite(o[:, [0, 1, 2, 3, 4, 5, 7]]).all() and np.isfinite(o[:, 8:]).all()
    if ortho:
        assert np.all(np.abs(norm3(o[:, CAM["d"]]) - 1.0) <= 16.0 * EPS), name
    u = rows[:, 4].astype(np.float64)
    assert np.all(np.abs(o[:, 7] - ((1.0 - u) * t0 + u * t1)) <= 4.0 * EPS * max(abs(t0), abs(t1))), name
    for spp in SPPS:                                   # the main ray does not depend on spp
        assert same_bits_or_both_nan(outs[spp][:, :8].astype(f32), o[:, :8].astype(f32)).all()
    if lens:                                           # the `sic` of camera/mod.rs:173: the y differential is built from dx_camera
        raw = camera_raw(be, cam, 4, rows)
        assert same_bits_or_both_nan(raw[:, CAM["ryd"]], raw[:, CAM["rxd"]]).all() and same_bits_or_both_nan(raw[:, CAM["ryo"]], raw[:, CAM["rxo"]]).all(), name
    else:                                              # the differentials are the main rays of the neighbouring pixels, shrunk toward the main ray by 1 / sqrt(spp)
        shift_x, shift_y = rows.copy(), rows.copy()
        shift_x[:, 0] += 1.0; shift_y[:, 1] += 1.0
        dx = camera_raw(be, cam, 1, shift_x).astype(np.float64)[:, CAM["d"]]
        dy = camera_raw(be, cam, 1, shift_y).astype(np.float64)[:, CAM["d"]]
        exact = np.abs(rows[:, 0:2] + 1.0 - (rows[:, 0:2].astype(np.float64) + 1.0)).max(axis=1) == 0.0     # p_film + 1 is itself a binary32
        for spp in SPPS:
            s = 1.0 / np.sqrt(spp)
            d = outs[spp][:, CAM["d"]]
            assert np.all(np.abs(outs[spp][:, CAM["rxd"]] - (d + (dx - d) * s))[exact] <= 8.0 * EPS), (name, spp)
            assert np.all(np.abs(outs[spp][:, CAM["ryd"]] - (d + (dy - d) * s))[exact] <= 8.0 * EPS), (name, spp)
            # the auxiliary origins are the pinhole itself; the main ray's went through Ray::transform's shift along d (transform.rs:307-322)
            size = np.abs(o[:, CAM["o"]]).max() + 1.0
            assert np.all(np.abs(outs[spp][:, CAM["rxo"]] - o[:, CAM["o"]]) <= 16.0 * EPS * size) and np.all(np.abs(outs[spp][:, CAM["ryo"]] - o[:, CAM["o"]]) <= 16.0 * EPS * size)


def check_lens_focus(be, name="thin_lens"):
    """with a thin lens the main ray and the x auxiliary ray (spp = 1) cross the plane of focus where the pinhole camera's main rays of p_film and
    p_film + (1, 0) cross it: all in camera space, through the binary64 inverse of camera-to-world"""
    cams = cameras(be)
    cam, _, _, _ = cams[name]
    pin = cams["pinhole"][0]
    rows = camera_rows(name, 82, 20000)
    rows[:, 0:2] = np.floor(rows[:, 0:2]) + 0.5          # p_film + 1 exact
    shifted = rows.copy(); shifted[:, 0] += 1.0
    o = camera_raw(be, cam, 1, rows).astype(np.float64)
    p0, p1 = camera_raw(be, pin, 1, rows).astype(np.float64), camera_raw(be, pin, 1, shifted).astype(np.float64)
    c2w, w2c = R.mat(cam.desc.camera_to_world)
    focal = float(cam.desc.focal_dist)

    def at_focus(org, d):
        oc, dc = R.tf_point(w2c, org), R.tf_vector(w2c, d)
        return oc + dc * ((focal - oc[:, 2]) / dc[:, 2])[:, None]
    tol = 64.0 * EPS * focal
    assert np.all(np.abs(at_focus(o[:, CAM["o"]], o[:, CAM["d"]]) - at_focus(p0[:, CAM["o"]], p0[:, CAM["d"]])) <= tol)
    assert np.all(np.abs(at_focus(o[:, CAM["rxo"]], o[:, CAM["rxd"]]) - at_focus(p1[:, CAM["o"]], p1[:, CAM["d"]])) <= tol)


def check_edge_table_reaches_the_edges(hook_of):
    """on the oracle: the table takes the binary64 edge-function fallback (a hit whose binary32 edge function is exactly 0), a sphere's second root
    and pole nudge, the coordinate_system frame (ns along ss), the zero-dn branch, and a singular solve_2x2"""
    # the fallback: rays through a vertex or along an edge whose binary32 edge functions hold an exact 0
    h = hook_of("det", "tri_plain")
    rows = edge_rows(h.targets)
    o = h(rows)
    g = h.targets[0]
    r32 = rows[:, 0:6]
    zero = np.zeros(len(rows), bool)
    with np.errstate(all="ignore"):
        d = r32[:, 3:6]
        kz = np.argmax(np.abs(d), axis=1); kx = (kz + 1) % 3; ky = (kx + 1) % 3
        i = np.arange(len(rows))
        pt = [(g.p[v].astype(f32) - r32[:, 0:3]) for v in range(3)]
        sx, sy = -d[i, kx] / d[i, kz], -d[i, ky] / d[i, kz]
        x = [q[i, kx] + sx * q[i, kz] for q in pt]; y = [q[i, ky] + sy * q[i, kz] for q in pt]
        for a, b in ((1, 2), (2, 0), (0, 1)):
            zero |= (x[a] * y[b] - y[a] * x[b]) == 0.0
    assert (zero & o["hit"]).sum() >= 3, "no hit went through the binary64 edge functions"
    assert (zero & ~o["hit"] & np.isfinite(rows[:, 0:6]).all(axis=1)).sum() >= 1
    # the second root and the pole nudge
    h = hook_of("det", "sph_partial")
    rows = edge_rows(h.targets)
    o = h(rows)
    g = h.targets[0]
    t0, t1 = g.roots(rows[:, 0:3].astype(np.float64), rows[:, 3:6].astype(np.float64))
    with np.errstate(all="ignore"):
        second = o["hit"] & (t0 > 1.0e-3) & (np.abs(o["t"] - t1) <= 1.0e-4 * np.abs(t1))
    assert second.sum() >= 2, "no clipped first root"
    h = hook_of("det", "sph_full")
    rows = edge_rows(h.targets)
    o = h(rows)
    g = h.targets[0]
    local = o["p"] - g.centre
    nudged = o["hit"] & (np.abs(local[:, 0] - 1.0e-5 * g.r) <= 1.0e-7 * g.r) & (local[:, 1] == 0.0)
    assert nudged.sum() >= 2, "no hit at a pole"
    # the coordinate_system frame and the zero-dn branch
    h = hook_of("det", "tri_tangent_along_normal")
    rows = edge_rows(h.targets)
    o = h(rows)
    o["hit"] &= ~undefined_by_the_reference(h.targets, rows)
    assert o["hit"].sum() > 10 and np.all(np.abs(norm3(o["s_dpdu"][o["hit"]]) - 1.0) < 1.0e-6)
    assert np.all(np.abs(dot3(o["ns"][o["hit"]], o["s_dpdu"][o["hit"]])) < 1.0e-6)
    h2 = hook_of("det", "tri_uv_degenerate_one_normal")
    rows2 = edge_rows(h2.targets)
    o2 = h2(rows2)
    o2["hit"] &= ~undefined_by_the_reference(h2.targets, rows2)
    assert o2["hit"].sum() > 10 and np.all(o2["dndu"][o2["hit"]] == 0.0) and np.all(o2["dndv"][o2["hit"]] == 0.0)
    h3 = hook_of("det", "tri_uv_degenerate_normals")
    rows3 = edge_rows(h3.targets)
    o3 = h3(rows3)
    o3["hit"] &= ~undefined_by_the_reference(h3.targets, rows3)
    assert np.all(np.abs(norm3(o3["dndu"][o3["hit"]]) - 1.0) < 1.0e-5), "coordinate_system(dn) gives unit vectors"
    # a singular system: the sliver's, and differentials along the surface
    h = hook_of("det", "tri_sliver")
    rows = edge_rows(h.targets)
    o = h(rows)
    m = o["hit"] & (rows[:, 9] != 0.0) & ~undefined_by_the_reference(h.targets, rows)
    assert m.sum() > 10 and np.all(o["dudx"][m] == 0.0) and np.all(o["dpdx"][m] == 0.0)
