"""A binary64 restatement of the reference's lights, written from the Rust (cited by file and line) and from neither C++ copy:
light/{point,distant,infinite,diffuse}.rs, sampling.rs Distribution1D/2D, shapes/mod.rs:39-66, the sample / intersect of
shapes/triangle.rs and shapes/sphere.rs, geometry/mod.rs (spherical_theta / phi, offset_ray_origin), the level-0 lookup of mipmap.rs.

It reads what a SceneBuilder holds (vertices, matrices, texels: the inputs of both libraries), never what a library computed.  Everything
is evaluated in binary64 on the binary32 inputs; where binary32 rounding may send the reference down another branch than binary64 (u at a
CDF entry, a direction at a cell edge, a ray grazing an edge or a limb, a root at the ray's origin) the row is flagged `fragile`."""
import numpy as np

PI = np.pi
EPS = 2.0 ** -24                                      # err_float.rs: MACHINE_EPSILON = f32::EPSILON / 2


def gamma(n):                                         # err_float.rs:7-10
    return n * EPS / (1.0 - n * EPS)


def dot(a, b): return np.sum(a * b, axis=-1)
def norm(a): return np.sqrt(dot(a, a))


def normalize(a):
    with np.errstate(all="ignore"):
        return a / norm(a)[..., None]


def cross(a, b): return np.cross(a, b)


def mat(t):
    """an ftn_transform's two matrices as [row][col] arrays (the flat arrays are cgmath's, column-major)"""
    return np.array(t.m[:], np.float64).reshape(4, 4).T, np.array(t.inv[:], np.float64).reshape(4, 4).T


def tf_point(m, p): return p @ m[:3, :3].T + m[:3, 3]
def tf_vector(m, v): return v @ m[:3, :3].T
def tf_normal(minv, n):
    """transform.rs:133-139 as written: x = invt[0][0] n.x + invt[1][0] n.y + invt[2][0] n.z with cgmath's m[column][row], which is row 0 of
    the inverse times n -- the inverse itself, not its transpose, whatever the comment there says"""
    return n @ minv[:3, :3].T


# ---------------------------------------------------------------- what a SceneBuilder holds
def world_bound(b):
    """the union of the shapes' world bounds: a triangle's is its vertices', a sphere's the transformed corners of its object bound
    (sphere.rs:61-63); -> the bounding sphere, bounds.rs:208-212: the centre and its distance to the maximum corner"""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    if b.P:
        P = np.concatenate(b.P).astype(np.float64)
        used = np.concatenate(b.tri_indices).ravel()
        lo, hi = np.minimum(lo, P[used].min(axis=0)), np.maximum(hi, P[used].max(axis=0))
    for s in b.spheres:
        m, _ = mat(s.object_to_world)
        c = np.array([[x, y, z] for x in (-s.radius, s.radius) for y in (-s.radius, s.radius) for z in (s.z_min, s.z_max)], np.float64)
        w = tf_point(m, c)
        lo, hi = np.minimum(lo, w.min(axis=0)), np.maximum(hi, w.max(axis=0))
    centre = (lo + hi) / 2.0
    return centre, float(norm(hi - centre))


def describe(b):
    """the lights of a SceneBuilder in Scene::new's order (scene/mod.rs:32-49): the explicit ones, then the area lights.  The scenes of
    tests/_light_common.py hold at most one emitting primitive, so the BVH's order does not enter."""
    _, radius = world_bound(b)
    out = []
    for l in b.lights:
        rgb, v = np.array(l.rgb[:], np.float64), np.array(l.v[:], np.float64)
        if l.type == 0:
            out.append(dict(kind="point", I=rgb, p=v))
        elif l.type == 1:
            out.append(dict(kind="distant", L=rgb, d=v, radius=radius))
        else:
            m, inv = mat(l.light_to_world)
            out.append(dict(kind="infinite", env=EnvLight(b.envmaps[l.envmap], m, inv), radius=radius))
    emitting = [p for p in b.prims if p[-1] >= 0]
    assert len(emitting) <= 1
    for p in b.prims:
        if p[0] == "trirange":
            _, first, nt, _, area = p
            if area >= 0:
                assert nt == 1
                out.append(dict(kind="area", L=np.array(b.area_emit[area], np.float64), shape=Triangle(b, first)))
        elif p[3] >= 0:
            out.append(dict(kind="area", L=np.array(b.area_emit[p[3]], np.float64), shape=Sphere(b.spheres[p[1]])))
    return out


# ---------------------------------------------------------------- sampling.rs:59-180
class Distribution1D:
    def __init__(self, func):                         # :84-107
        self.func = np.asarray(func, np.float64)
        n = len(self.func)
        with np.errstate(all="ignore"):
            cdf = np.concatenate([[0.0], np.cumsum(self.func / n)])
            self.integral = cdf[n]
            # :96-100: only cdf[1..] is rewritten, cdf[0] stays 0 whatever the integral is (a NaN integral leaves one finite entry)
            self.cdf = np.arange(n + 1) / n if self.integral == 0.0 else np.concatenate([[0.0], cdf[1:] / self.integral])
        self.n = n

    def search(self, u):
        """search_sorted(cdf.len(), |i| cdf[i] <= u), :66-81: first = the bisection's count of entries <= u (on an array that is not sorted,
        as with a NaN in it, the bisection's own answer), then (first - 1).clamp(0, size - 2).  first == 0 (u < 0 or NaN: not even cdf[0] = 0
        is <= u) makes `first - 1` underflow a usize: a panic in a debug build, size - 2 after wrapping in a release one.  Both C++ copies return
        cell 0 there, and so does this: a pinned deviation, flagged in `underflow` by sample_continuous"""
        size = self.n + 1
        first = np.zeros(u.shape, np.int64)
        length = np.full(u.shape, size, np.int64)
        while np.any(length > 0):
            live = length > 0
            half = length >> 1
            mid = np.minimum(first + half, size - 1)
            with np.errstate(invalid="ignore"):
                key = (self.cdf[mid] <= u) & live
            first = np.where(key, mid + 1, first)
            length = np.where(key, length - (half + 1), np.where(live, half, length))
        return np.clip(first - 1, 0, size - 2)

    def sample_continuous(self, u):                   # :121-134 -> x, pdf, idx
        idx = self.search(u)
        lo, hi = self.cdf[idx], self.cdf[idx + 1]
        with np.errstate(all="ignore"):
            du = u - lo
            du = np.where(hi - lo > 0.0, du / np.where(hi - lo > 0.0, hi - lo, 1.0), du)
            pdf = self.func[idx] / self.integral
        return (idx + du) / self.n, pdf, idx

    def near_an_entry(self, u, ulps):
        """u within `ulps` binary32 ulps (of 1) of some CDF entry: the binary32 CDF is a running sum of up to n roundings"""
        c = self.cdf[np.isfinite(self.cdf)]
        if len(c) < 2:
            return np.zeros(u.shape, bool)
        k = np.clip(np.searchsorted(np.sort(c), u), 1, len(c) - 1)
        s = np.sort(c)
        return np.minimum(np.abs(u - s[k - 1]), np.abs(u - s[k])) <= ulps * 2.0 ** -23


class Distribution2D:
    def __init__(self, func, nu, nv):                 # :144-161
        self.cond = [Distribution1D(func[v * nu:(v + 1) * nu]) for v in range(nv)]
        self.marg = Distribution1D([c.integral for c in self.cond])
        self.nu, self.nv = nu, nv
        self.func = np.asarray(func, np.float64).reshape(nv, nu)

    def sample_continuous(self, u):                   # :163-169 -> d0, d1, pdf, iu, iv, fragile
        d1, pdf1, iv = self.marg.sample_continuous(u[:, 1])
        d0, pdf0, iu = np.zeros(len(u)), np.zeros(len(u)), np.zeros(len(u), np.int64)
        fragile = self.marg.near_an_entry(u[:, 1], 16)
        for v in np.unique(iv):
            take = iv == v
            d0[take], pdf0[take], iu[take] = self.cond[v].sample_continuous(u[take, 0])
            fragile[take] |= self.cond[v].near_an_entry(u[take, 0], 16)
        return d0, d1, pdf0 * pdf1, iu, iv, fragile

    def pdf(self, p):                                 # :171-179 -> pdf, iu, iv, fragile  (`as usize` saturates and sends NaN to 0)
        with np.errstate(all="ignore"):
            x, y = p[:, 0] * self.nu, p[:, 1] * self.nv
            iu = np.clip(np.where(np.isnan(x), 0.0, x), 0, self.nu - 1).astype(np.int64)
            iv = np.clip(np.where(np.isnan(y), 0.0, y), 0, self.nv - 1).astype(np.int64)
            value = self.func[iv, iu] / self.marg.integral
            # acos / atan2 in binary32 and the product are good to a few ulp of the cell coordinate
            fragile = (np.abs(x - np.round(x)) <= 32 * 2.0 ** -23 * np.maximum(np.abs(x), 1.0)) | (np.abs(y - np.round(y)) <= 32 * 2.0 ** -23 * np.maximum(np.abs(y), 1.0))
        return value, iu, iv, fragile


# ---------------------------------------------------------------- geometry/mod.rs:23-34, :64-85
def spherical_theta(v): return np.arccos(np.clip(v[:, 2], -1.0, 1.0))


def spherical_phi(v):
    p = np.arctan2(v[:, 1], v[:, 0])
    return np.where(p < 0.0, p + 2.0 * PI, p)


def offset_ray_origin(p, p_err, n, w):
    """:72-85, the sum rounded to binary32 and stepped to the next binary32 away from the surface as there (at coordinates of 1e4 that step is 1e-3)"""
    d = dot(np.abs(n), p_err)
    off = d[:, None] * n
    off = np.where((dot(w, n) < 0.0)[:, None], -off, off)
    with np.errstate(all="ignore"):
        po = (p + off).astype(np.float32)
        po = np.where(off > 0.0, np.nextafter(po, np.float32(np.inf)), np.where(off < 0.0, np.nextafter(po, np.float32(-np.inf)), po))
    return po.astype(np.float64)


# ---------------------------------------------------------------- mipmap.rs:245-312 (level 0, ImageWrap::Repeat), light/infinite.rs
class EnvLight:
    def __init__(self, texels, l2w, w2l):
        self.tex = np.asarray(texels, np.float64)     # [t][s][c]: `resolution` is (s size, t size) = (w, h)
        self.h, self.w = self.tex.shape[:2]
        self.l2w, self.w2l = l2w, w2l                 # new_envmap :28-29: world_to_light = light_to_world.inverse()
        self.distribution = self.compute_distribution()

    def texel(self, s, t):                            # mipmap.rs:297-312: rem_euclid
        return self.tex[np.mod(t, self.h), np.mod(s, self.w)]

    def triangle(self, st, scale=False):
        """mipmap.rs:265-279 at level 0.  scale: also the largest |component| of the four texels blended (what the rounding error is relative to)"""
        with np.errstate(all="ignore"):
            s, t = st[:, 0] * self.w - 0.5, st[:, 1] * self.h - 0.5
            sat = lambda x: np.clip(np.where(np.isnan(x), 0.0, x), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)      # `as i32`
            s0, t0 = sat(np.floor(s)), sat(np.floor(t))
            ds, dt = (s - s0)[:, None], (t - t0)[:, None]
            four = [self.texel(s0, t0), self.texel(s0, t0 + 1), self.texel(s0 + 1, t0), self.texel(s0 + 1, t0 + 1)]
            value = four[0] * (1.0 - ds) * (1.0 - dt) + four[1] * (1.0 - ds) * dt + four[2] * ds * (1.0 - dt) + four[3] * ds * dt
            if scale:
                return value, np.nan_to_num(np.abs(np.stack(four)), nan=0.0, posinf=0.0).max(axis=(0, 2))
            return value

    def compute_distribution(self):
        """infinite.rs:63-78.  `let (height, width) = mipmap.resolution()` binds the map's WIDTH to `height` and its height to `width`: the
        distribution of a w x h map has h columns and w rows, and its row j is filled from v = j / w.  lookup_trilinear_width(st, 1 / max(w, h))
        (mipmap.rs:245-257): one level and level 0 >= levels - 1 for a 1 x 1 map -> its texel; a level below 0 unless max(w, h) is a power of
        two -> triangle(0); exactly 0 for a power of two -> lerp(0, triangle(0), triangle(1)) = triangle(0) as long as level 1 is finite
        (the maps of the tests with a non-finite texel have widths that are no power of two)."""
        height, width = self.w, self.h
        j, i = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
        st = np.stack([(i / width).ravel(), (j / height).ravel()], axis=1)
        rgb = np.broadcast_to(self.tex[0, 0], (len(st), 3)) if (self.w, self.h) == (1, 1) else self.triangle(st)
        lum = rgb[:, 0] * 0.212671 + rgb[:, 1] * 0.715160 + rgb[:, 2] * 0.072169            # spectrum/mod.rs:104-107
        img = lum * np.sin(PI * (j.ravel() + 0.5) / height)
        return Distribution2D(img, width, height)

    def sample(self, ref_p, time, u, radius):         # infinite.rs:99-140
        d0, d1, map_pdf, iu, iv, fragile = self.distribution.sample_continuous(u)
        theta, phi = d1 * PI, d0 * 2.0 * PI
        local = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], axis=1)
        wi = tf_vector(self.l2w, local)
        with np.errstate(all="ignore"):
            pdf = np.where(np.sin(theta) == 0.0, 0.0, map_pdf / (2.0 * PI * PI * np.sin(theta)))
        unimplemented = map_pdf == 0.0                # :101-103 unimplemented!(): pinned as pdf 0 (test_light_cpu.py)
        pdf = np.where(unimplemented, 0.0, pdf)
        radiance, scale = self.triangle(np.stack([d0, d1], axis=1), scale=True)           # lookup_trilinear_width(uv, 0.0): level < 0 for fewer than 28 levels
        return dict(radiance=radiance, wi=wi, pdf=pdf, p1_p=ref_p + wi * (2.0 * radius), p1_perr=np.zeros_like(wi), p1_n=np.zeros_like(wi),
                    p1_time=time, cell=np.stack([iu, iv], axis=1), uv=np.stack([d0, d1], axis=1), fragile=fragile, unimplemented=unimplemented, radiance_scale=scale,
                    underflow=~(u[:, 0] >= 0.0) | ~(u[:, 1] >= 0.0))

    def pdf(self, wi):                                # infinite.rs:142-154 -> pdf, cell, fragile
        w = tf_vector(self.w2l, wi)
        theta, phi = spherical_theta(w), spherical_phi(w)
        value, iu, iv, fragile = self.distribution.pdf(np.stack([phi * (1.0 / (2.0 * PI)), theta * (1.0 / PI)], axis=1))
        with np.errstate(all="ignore"):
            pdf = np.where(np.sin(theta) == 0.0, 0.0, value / (2.0 * PI * PI * np.sin(theta)))
        # sin(theta) == 0 decides differently in binary32 at the poles (sin of binary32's pi is -8.7e-8, not 0)
        fragile = fragile | (np.abs(w[:, 2]) >= norm(w) * (1.0 - 1.0e-6)) | ~np.isfinite(norm(w))
        return pdf, np.stack([iu, iv], axis=1), fragile

    def Le(self, d):                                  # infinite.rs:156-164 -> radiance, largest texel blended
        w = normalize(tf_vector(self.w2l, d))
        return self.triangle(np.stack([spherical_phi(w) * (1.0 / (2.0 * PI)), spherical_theta(w) * (1.0 / PI)], axis=1), scale=True)


# ---------------------------------------------------------------- shapes/triangle.rs
class Triangle:
    def __init__(self, b, tri):
        idx = np.concatenate(b.tri_indices)[tri]
        mesh = b.meshes[int(np.concatenate(b.tri_mesh)[tri])]
        P = np.concatenate(b.P).astype(np.float64)
        self.p = P[idx]
        self.n = np.concatenate(b.N).astype(np.float64)[idx] if mesh.has_normals else None
        self.uv = np.concatenate(b.UV).astype(np.float64)[idx] if mesh.has_uvs else np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0]])   # :131-143
        self.flip = bool(mesh.flip_normals)

    def area(self):                                   # :171-174
        p0, p1, p2 = self.p
        return 0.5 * norm(cross(p1 - p0, p2 - p0))

    def sample(self, u):                              # :395-420, sampling.rs:48-51
        p0, p1, p2 = self.p
        su0 = np.sqrt(u[:, 0])
        b0, b1 = (1.0 - su0)[:, None], (u[:, 1] * su0)[:, None]
        b2 = 1.0 - b0 - b1
        p = b0 * p0 + b1 * p1 + b2 * p2
        n = normalize(cross(p1 - p0, p2 - p0))
        fragile = np.zeros(len(u), bool)
        if self.n is not None:
            ns = normalize(b0 * self.n[0] + b1 * self.n[1] + b2 * self.n[2])
            d = dot(np.broadcast_to(n, ns.shape), ns)
            fragile |= np.abs(d) <= 1.0e-5
            sn = np.where((d < 0.0)[:, None], -n, n)
        else:
            sn = np.broadcast_to(-n if self.flip else n, p.shape)
        p_err = gamma(6) * (np.abs(b0 * p0) + np.abs(b1 * p1) + np.abs(b2 * p2))
        return dict(p=p, p_err=p_err, n=np.array(sn), bary=np.concatenate([b0, b1, b2], axis=1), fragile=fragile)

    def hit_test(self, o, d, t_max=np.inf, exact_origin=False):
        """the hit test of :176-268 and the late `None` of :277-288 -> dict(miss, bary, t, delta_t, fragile, nan_edges): fragile = binary32 may
        decide otherwise; delta_t = the reference's own bound on t's error (:252-268, in binary64); nan_edges = an edge function is NaN
        (sign_differs, :428-434, then goes by the NaN's sign bit, which IEEE 754 leaves to the implementation: hit or miss is not defined by the
        reference's text).  exact_origin: the origin is a binary32 number both sides use as it is (a ray batch), not a rounded sum (a spawned ray):
        the origin's half ulp is then left out of `fragile`."""
        p0, p1, p2 = self.p
        with np.errstate(all="ignore"):
            pt = np.stack([p0 - o, p1 - o, p2 - o], axis=1)                           # [row][vertex][xyz]
            kz = np.argmax(np.abs(d), axis=1)                                          # max_dimension
            kx = (kz + 1) % 3
            ky = (kx + 1) % 3
            r = np.arange(len(o))
            perm = lambda a: np.stack([a[r, kx], a[r, ky], a[r, kz]], axis=-1)
            dp = perm(d)
            pt = np.stack([perm(pt[:, k]) for k in range(3)], axis=1)
            sx, sy, sz = -dp[:, 0] / dp[:, 2], -dp[:, 1] / dp[:, 2], 1.0 / dp[:, 2]
            x = pt[:, :, 0] + sx[:, None] * pt[:, :, 2]
            y = pt[:, :, 1] + sy[:, None] * pt[:, :, 2]
            e0 = x[:, 1] * y[:, 2] - y[:, 1] * x[:, 2]
            e1 = x[:, 2] * y[:, 0] - y[:, 2] * x[:, 0]
            e2 = x[:, 0] * y[:, 1] - y[:, 0] * x[:, 1]
            e = np.stack([e0, e1, e2], axis=1)
            differs = (e.min(axis=1) < 0.0) & (e.max(axis=1) > 0.0)                    # sign_differs
            det = e0 + e1 + e2
            z = pt[:, :, 2] * sz[:, None]
            t_scaled = e0 * z[:, 0] + e1 * z[:, 1] + e2 * z[:, 2]
            miss = differs | (det == 0.0) | ((det < 0.0) & ((t_scaled >= 0.0) | (t_scaled < t_max * det))) | ((det > 0.0) & ((t_scaled <= 0.0) | (t_scaled > t_max * det)))
            inv = 1.0 / det
            bary = e * inv[:, None]
            t = t_scaled * inv
            # the conservative t > 0 test, :252-268
            max_z, max_x, max_y = np.abs(z).max(axis=1), np.abs(x).max(axis=1), np.abs(y).max(axis=1)
            delta_x, delta_y, delta_z = gamma(5) * (max_x + max_z), gamma(5) * (max_y + max_z), gamma(3) * max_z
            delta_e = 2.0 * (gamma(2) * max_x * max_y + delta_y * max_x + delta_x * max_y)
            max_e = np.abs(e).max(axis=1)
            delta_t = 3.0 * (gamma(3) * max_e * max_z + delta_e * max_z + delta_z * max_e) * np.abs(inv)
            miss |= t <= delta_t
            # degenerate uvs on a degenerate triangle, :277-288
            duv02, duv12 = self.uv[0] - self.uv[2], self.uv[1] - self.uv[2]
            if abs(duv02[0] * duv12[1] - duv02[1] * duv12[0]) < 1.0e-8 and dot(cross(p2 - p0, p1 - p0), cross(p2 - p0, p1 - p0)) == 0.0:
                miss |= True
            # grazing an edge: an edge function within binary32's reach of 0 (each is a difference of two products of the sheared coordinates)
            # and the origin itself is a rounded sum: half an ulp of its largest coordinate in every translated vertex
            scale = max_x * max_y
            if exact_origin:
                # what binary32 still rounds: p - o, the shear's product and its sum, each to half an ulp of its own size -- which a ray aimed at
                # a small triangle from far away cancels down to the triangle's size (|p - o| = 2^38 towards a triangle of 0.25: all three
                # edge functions are 0 in binary32)
                mag_x = (np.abs(pt[:, :, 0]) + np.abs(sx[:, None] * pt[:, :, 2])).max(axis=1)
                mag_y = (np.abs(pt[:, :, 1]) + np.abs(sy[:, None] * pt[:, :, 2])).max(axis=1)
                origin_term = 4.0 * EPS * (mag_x * max_y + mag_y * max_x)
            else:
                ulp_o = 2.0 * EPS * np.abs(o).max(axis=1)
                origin_term = 4.0 * ulp_o * (max_x + max_y)
            edge_reach = 64 * EPS * scale + origin_term
            fragile = (np.abs(e).min(axis=1) <= edge_reach) | (np.abs(t - delta_t) <= 1.0e-3 * np.abs(delta_t) + 64 * EPS * np.abs(t)) | ~np.isfinite(det)
            fragile |= (np.abs(t_scaled) <= 64 * EPS * max_e * max_z) & ~(np.abs(t) < 0.5 * delta_t)     # (a t well inside delta_t is a miss whatever its sign)
            fragile |= np.isfinite(t_max) & (np.abs(t - t_max) <= 64 * EPS * (np.abs(t_max) + max_e * max_z * np.abs(inv)))      # t_scaled against t_max * det
            if exact_origin:
                # two edge functions of opposite sign, each beyond binary32's reach: sign_differs says so in binary32 as well, whatever the third
                # one, t and det come to (a ray batch against every primitive of a scene: nearly every pair is such a miss, and the third edge
                # function of a small triangle far off the ray is within reach of 0 more often than not)
                fragile &= ~((e.max(axis=1) > edge_reach) & (e.min(axis=1) < -edge_reach))
            # the same edge functions in binary32, where 3e20 squared is already infinite and inf - inf is NaN
            f = np.float32
            x32 = pt[:, :, 0].astype(f) + (-dp[:, 0].astype(f) / dp[:, 2].astype(f))[:, None] * pt[:, :, 2].astype(f)
            y32 = pt[:, :, 1].astype(f) + (-dp[:, 1].astype(f) / dp[:, 2].astype(f))[:, None] * pt[:, :, 2].astype(f)
            e32 = np.stack([x32[:, 1] * y32[:, 2] - y32[:, 1] * x32[:, 2], x32[:, 2] * y32[:, 0] - y32[:, 2] * x32[:, 0], x32[:, 0] * y32[:, 1] - y32[:, 0] * x32[:, 1]], axis=1)
        return dict(miss=miss, bary=bary, t=t, delta_t=delta_t, inv_det=inv, fragile=fragile, nan_edges=np.isnan(e).any(axis=1) | np.isnan(e32).any(axis=1))

    def intersect(self, o, d):
        """:176-393 for a ray with t_max = infinity -> hit, p, n, fragile, whether an edge function is NaN"""
        p0, p1, p2 = self.p
        h = self.hit_test(o, d)
        bary, fragile = h["bary"], h["fragile"]
        with np.errstate(all="ignore"):
            p = bary[:, 0:1] * p0 + bary[:, 1:2] * p1 + bary[:, 2:3] * p2
            n = normalize(cross(p0 - p2, p1 - p2))
            if self.flip:
                n = -n
            n = np.broadcast_to(n, p.shape)
            if self.n is not None:                                                     # :332-391: hit.n = faceforward(hit.n, ns)
                ns = normalize(bary[:, 0:1] * self.n[0] + bary[:, 1:2] * self.n[1] + bary[:, 2:3] * self.n[2])
                dd = dot(n, ns)
                fragile = fragile | (np.abs(dd) <= 1.0e-5)
                n = np.where((dd < 0.0)[:, None], -n, n)
        return ~h["miss"], p, np.array(n), fragile, h["nan_edges"]


# ---------------------------------------------------------------- shapes/sphere.rs
class Sphere:
    def __init__(self, s):
        self.o2w, self.o2w_inv = mat(s.object_to_world)
        self.w2o, _ = mat(s.world_to_object)
        self.r, self.z_min, self.z_max = float(s.radius), float(s.z_min), float(s.z_max)
        self.theta_min, self.theta_max, self.phi_max = float(s.theta_min), float(s.theta_max), float(s.phi_max)
        self.rev = bool(s.reverse_orientation)

    def area(self):                                   # :77-79
        return self.phi_max * self.r * (self.z_max - self.z_min)

    def sample(self, u):                              # :202-218, sampling.rs:37-42: the WHOLE sphere, whatever z_min / z_max / phi_max say
        z = 1.0 - 2.0 * u[:, 0]
        rr = np.sqrt(np.maximum(1.0 - z * z, 0.0))
        phi = 2.0 * PI * u[:, 1]
        p_obj = self.r * np.stack([rr * np.cos(phi), rr * np.sin(phi), z], axis=1)
        n = normalize(tf_normal(self.o2w_inv, p_obj))
        if self.rev:
            n = -n
        p_obj = p_obj * (self.r / norm(p_obj))[:, None]
        err = gamma(5) * np.abs(p_obj)
        m = self.o2w                                  # transform.rs:245-264
        p_err = (gamma(3) + 1.0) * (err @ np.abs(m[:3, :3]).T) + gamma(3) * (np.abs(p_obj) @ np.abs(m[:3, :3]).T + np.abs(m[:3, 3]))
        return dict(p=tf_point(m, p_obj), p_err=p_err, n=n, obj=p_obj, fragile=np.zeros(len(u), bool))

    def clipped(self, p, phi):                        # :121-123
        return ((self.z_min > -self.r) & (p[:, 2] < self.z_min)) | ((self.z_max < self.r) & (p[:, 2] > self.z_max)) | (phi > self.phi_max)

    def near_a_clip(self, p, phi):
        tol = 1.0e-5
        f = np.zeros(len(p), bool)
        if self.z_min > -self.r:
            f |= np.abs(p[:, 2] - self.z_min) <= tol * self.r
        if self.z_max < self.r:
            f |= np.abs(p[:, 2] - self.z_max) <= tol * self.r
        f |= np.abs(phi - self.phi_max) <= tol
        if self.phi_max < 2.0 * PI:                   # the seam phi = 0 borders the cut as well
            f |= (phi <= tol) | (phi >= 2.0 * PI - tol)
        return f

    def at(self, o, d, t):                            # :112-117
        with np.errstate(all="ignore"):
            p = o + d * t[:, None]
            p = p * (self.r / norm(p))[:, None]
            on_axis = (p[:, 0] == 0.0) & (p[:, 1] == 0.0)
            p[:, 0] = np.where(on_axis, 1.0e-5 * self.r, p[:, 0])
            phi = np.arctan2(p[:, 1], p[:, 0])
            return p, np.where(phi < 0.0, phi + 2.0 * PI, phi)

    def intersect(self, o_w, d_w, t_max=np.inf):
        """:83-200 -> hit, p, n, fragile, which root (0 near, 1 far), the object-space point, t, the object-space ray (o, d).  The EFloat intervals of
        the reference are not restated: a root within their reach of 0 or of t_max, or a discriminant within reach of 0, flags the row instead."""
        with np.errstate(all="ignore"):
            m = self.w2o
            o, d = tf_point(m, o_w), tf_vector(m, d_w)
            o_err = gamma(3) * (np.abs(o_w) @ np.abs(m[:3, :3]).T + np.abs(m[:3, 3]))   # transform.rs:230-243, :286-299
            len_sq = dot(d, d)
            dt = np.where(len_sq > 0.0, dot(np.abs(d), o_err) / len_sq, 0.0)
            o = o + d * dt[:, None]
            t_max = t_max - dt                        # transform.rs:307-322
            a, b, c = len_sq, 2.0 * dot(d, o), dot(o, o) - self.r * self.r
            disc = b * b - 4.0 * a * c                # math.rs:36-53
            miss = disc < 0.0
            root = np.sqrt(np.maximum(disc, 0.0))
            q = np.where(b < 0.0, -0.5 * (b - root), -0.5 * (b + root))
            ta, tb = q / a, c / q
            t0, t1 = np.minimum(ta, tb), np.maximum(ta, tb)
            # what the error intervals can reach: the terms of c are of size |o|^2 + r^2, the roots of size (|o| + r) / |d|
            size = (norm(o) + self.r) / np.sqrt(len_sq)
            reach = 1.0e-4 * size
            fragile = (np.abs(disc) <= 3.0e-6 * (b * b + np.abs(4.0 * a * c))) | ~np.isfinite(disc) | ~(len_sq > 0.0)
            miss |= (t1 <= 0.0) | (t0 > t_max)        # :99-101
            fragile |= np.abs(t0 - t_max) <= reach
            fragile |= np.abs(t1) <= reach
            far = t0 <= 0.0                           # :104-110
            fragile |= np.abs(t0) <= reach
            t = np.where(far, t1, t0)
            miss |= far & (t1 > t_max)                # :104-110
            fragile |= np.abs(t1 - t_max) <= reach
            p, phi = self.at(o, d, t)
            clip = self.clipped(p, phi)
            fragile |= self.near_a_clip(p, phi) & ~miss
            miss |= clip & far                        # :125
            p2, phi2 = self.at(o, d, t1)
            second = clip & ~far
            clip2 = self.clipped(p2, phi2)
            fragile |= second & self.near_a_clip(p2, phi2) & ~miss
            miss |= second & (clip2 | (t1 > t_max))
            p = np.where(second[:, None], p2, p)
            t = np.where(second, t1, t)
            which = (far | second).astype(int)
            # the normal: dpdu x dpdv of :155-168, reversed at :183-185, then SurfaceHit::transform (transform.rs:340-346)
            theta = np.arccos(np.clip(p[:, 2] / self.r, -1.0, 1.0))
            zr = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2)
            cphi, sphi = p[:, 0] / zr, p[:, 1] / zr
            dpdu = np.stack([-self.phi_max * p[:, 1], self.phi_max * p[:, 0], np.zeros(len(p))], axis=1)
            dpdv = (self.theta_max - self.theta_min) * np.stack([p[:, 2] * cphi, p[:, 2] * sphi, -self.r * np.sin(theta)], axis=1)
            n = normalize(cross(dpdu, dpdv))
            if self.rev:
                n = -n
            n = normalize(tf_normal(self.o2w_inv, n))
            fragile |= zr <= 1.0e-4 * self.r          # at the poles dpdu vanishes
        return ~miss, tf_point(self.o2w, p), n, fragile, which, p, t, (o, d)


# ---------------------------------------------------------------- light/*.rs
def evaluate(light, rows):
    """one light of describe() on rows of tests/_light_common.py -> every output of the hook in binary64, `fragile`, and the discrete outcomes"""
    r = np.asarray(rows, np.float64)
    p, p_err, n, time, wi_in, u = r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9], r[:, 10:13], r[:, 13:15]
    m = len(r)
    z3 = np.zeros((m, 3))
    out = dict(fragile=np.zeros(m, bool), le=z3.copy())
    kind = light["kind"]
    if kind == "point":                               # point.rs:43-62
        d = light["p"] - p
        with np.errstate(all="ignore"):
            out.update(radiance=light["I"] / dot(d, d)[:, None], wi=normalize(d), pdf=np.ones(m), p1_p=np.broadcast_to(light["p"], (m, 3)), p1_perr=z3, p1_n=z3,
                       p1_time=time, pdf_in=np.zeros(m), pdf_s=np.zeros(m))
    elif kind == "distant":                           # distant.rs:49-71
        out.update(radiance=np.broadcast_to(light["L"], (m, 3)), wi=np.broadcast_to(light["d"], (m, 3)), pdf=np.ones(m), p1_p=p + light["d"] * (2.0 * light["radius"]),
                   p1_perr=z3, p1_n=z3, p1_time=time, pdf_in=np.zeros(m), pdf_s=np.zeros(m))
    elif kind == "infinite":
        env = light["env"]
        s = env.sample(p, time, u, light["radius"])
        pdf_in, cell_in, frag_in = env.pdf(wi_in)
        pdf_s, cell_s, frag_s = env.pdf(s["wi"])
        out.update({k: s[k] for k in ("radiance", "wi", "pdf", "p1_p", "p1_perr", "p1_n", "p1_time", "unimplemented", "uv", "radiance_scale", "underflow")})
        le, le_scale = env.Le(wi_in)
        out.update(pdf_in=pdf_in, pdf_s=pdf_s, le=le, le_scale=le_scale, cell=s["cell"], cell_in=cell_in, cell_s=cell_s,
                   fragile=s["fragile"] | frag_in, fragile_s=frag_s, same_cell=np.all(cell_s == s["cell"], axis=1))
    else:                                             # diffuse.rs:44-50, :74-93; shapes/mod.rs:51-66
        shape = light["shape"]
        s = shape.sample(u)
        with np.errstate(all="ignore"):
            wi = normalize(s["p"] - p)
            cosine = dot(s["n"], -wi)
            radiance = np.where((cosine > 0.0)[:, None], light["L"], 0.0)
        out["fragile"] |= s["fragile"] | (np.abs(cosine) <= 1.0e-5)
        pdfs = []
        for w in (wi_in, wi):
            o = offset_ray_origin(p, p_err, n, w)
            res = shape.intersect(o, w)
            hit, hp, hn, frag = res[:4]
            with np.errstate(all="ignore"):
                d = p - hp
                pdf = dot(d, d) / (np.abs(dot(hn, -w)) * shape.area())
            pdfs.append((np.where(hit, pdf, 0.0), hit, frag, res))
        out.update(radiance=radiance, wi=wi, pdf=pdfs[1][0], p1_p=s["p"], p1_perr=s["p_err"], p1_n=s["n"], p1_time=np.zeros(m), pdf_in=pdfs[0][0], pdf_s=pdfs[1][0],
                   le=radiance, hit_in=pdfs[0][1], hit_s=pdfs[1][1], sample=s)
        out["fragile"] |= pdfs[0][2] | pdfs[1][2]
        if isinstance(shape, Sphere):
            out["which_s"] = pdfs[1][3][4]
        else:
            out["nan_edges_in"], out["nan_edges_s"] = pdfs[0][3][4], pdfs[1][3][4]
    return out
