"""An independent binary64 restatement of the reference's texture path, written from the Rust: mipmap.rs (MIPMap::new, lookup_trilinear,
lookup_trilinear_width, triangle, get_texel_from_level), texture/{mapping,uv,checkerboard,image}.rs, the parameter handling of
material/{matte,plastic,metal,glass}.rs, OrenNayar::new (reflection/mod.rs) and roughness_to_alpha (reflection/microfacet.rs).  The pyramid
levels >= 1 come from the `resize` crate (Type::Triangle), which the reference does not vendor: resize_triangle() follows that crate's published
algorithm (separable; the filter's support of 1.0 is scaled by the ratio when shrinking; per output sample the taps are clamped to the image
and normalised).

It reads only what a SceneBuilder holds (textures, images, materials, material_textures) and shares no code with oracle/ or fountain_amd/csrc.
Everything is float64 over the float32 inputs; where the reference converts a float to an integer (`as i32`: saturating, NaN -> 0; i32 `+`
wrapping in release builds) the same is done here, so that rows far outside the image mean the same on both sides.  DESIGN.md 3.4."""
import numpy as np

from fountain_amd import _abi as A

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
ULPS_NEAR_INTEGER = 4        # a checkerboard / UV coordinate this close (in binary32 ulps of the coordinate) to an integer is fragile
BLACK_TOP_LEVEL = 1.0e-5     # ... and, in `black` mode, a level this close to n_levels - 1
MAX_FRAGILE_SHARE = 0.005


def as_i32(x):
    """Rust's `f as i32`"""
    x = np.asarray(x, np.float64)
    return np.where(np.isnan(x), 0.0, np.clip(x, I32_MIN, I32_MAX)).astype(np.int64)


def wrap_i32(x):
    return (x - I32_MIN) % (2 ** 32) + I32_MIN


# ---------------------------------------------------------------- MIPMap::new
def _shrink_axis0(a, n_dst):
    """resize, Type::Triangle, along axis 0: a[n_src, ...] -> [n_dst, ...]"""
    n_src = a.shape[0]
    ratio = n_src / n_dst
    scale = max(ratio, 1.0)
    radius = np.ceil(scale)
    centre = (np.arange(n_dst) + 0.5) * ratio - 0.5
    lo = np.clip(np.ceil(centre - radius), 0, n_src - 1).astype(np.int64)
    hi = np.clip(np.floor(centre + radius), 0, n_src - 1).astype(np.int64)
    out = np.zeros((n_dst,) + a.shape[1:])
    total = np.zeros(n_dst)
    for k in range(int((hi - lo).max()) + 1):
        idx = np.minimum(lo + k, hi)
        w = np.where(lo + k <= hi, np.maximum(1.0 - np.abs((idx - centre) / scale), 0.0), 0.0)
        total += w
        out += a[idx] * w.reshape((-1,) + (1,) * (a.ndim - 1))
    return out / total.reshape((-1,) + (1,) * (a.ndim - 1))


def pyramid(img):
    """MIPMap::new: img [h, w, 3] (row 0 = t 0) -> the list of levels, 1 + floor(log2(max(w, h))) of them"""
    cur = np.asarray(img, np.float64)
    h, w = cur.shape[:2]
    n_levels = 1 + int(max(w, h)).bit_length() - 1
    levels = [cur]
    for _ in range(1, n_levels):
        h, w = max(1, h // 2), max(1, w // 2)
        cur = _shrink_axis0(cur, h)
        cur = np.swapaxes(_shrink_axis0(np.swapaxes(cur, 0, 1), w), 0, 1)
        levels.append(cur)
    return levels


# ---------------------------------------------------------------- MIPMap lookups
class Mip:
    def __init__(self, texels, wrap):
        self.levels, self.wrap = pyramid(texels), wrap
        self.largest = float(np.nanmax(np.abs(np.where(np.isfinite(texels), texels, 0.0)))) if np.size(texels) else 0.0

    def texel(self, level, s, t):
        L = self.levels[level]
        h, w = L.shape[:2]
        if self.wrap == A.FTN_WRAP_REPEAT:
            return L[t % h, s % w]
        if self.wrap == A.FTN_WRAP_CLAMP:
            return L[np.clip(t, 0, h - 1), np.clip(s, 0, w - 1)]
        inside = (s >= 0) & (s < w) & (t >= 0) & (t < h)
        return np.where(inside[:, None], L[np.clip(t, 0, h - 1), np.clip(s, 0, w - 1)], 0.0)

    def triangle(self, level, st):
        level = min(max(level, 0), len(self.levels) - 1)
        h, w = self.levels[level].shape[:2]
        s, t = st[:, 0] * w - 0.5, st[:, 1] * h - 0.5
        s0, t0 = as_i32(np.floor(s)), as_i32(np.floor(t))
        ds, dt = (s - s0)[:, None], (t - t0)[:, None]
        s1, t1 = wrap_i32(s0 + 1), wrap_i32(t0 + 1)
        return (self.texel(level, s0, t0) * (1 - ds) * (1 - dt) + self.texel(level, s0, t1) * (1 - ds) * dt +
                self.texel(level, s1, t0) * ds * (1 - dt) + self.texel(level, s1, t1) * ds * dt)

    def lookup_width(self, st, width):
        """-> value [n, 3], branch [n] (0 = level 0 alone, 1 = two levels, 2 = the top texel), level [n]"""
        n_levels = len(self.levels)
        with np.errstate(all="ignore"):
            wd = np.where(np.isnan(width), 1.0e-8, np.maximum(width, np.float64(np.float32(1.0e-8))))     # f32::max keeps the number
            level = n_levels - 1.0 + np.log2(wd)
            branch = np.where(level < 0.0, 0, np.where(level >= n_levels - 1, 2, 1))
            out = np.zeros((st.shape[0], 3))
            m = branch == 0
            if m.any():
                out[m] = self.triangle(0, st[m])
            m = branch == 2
            if m.any():
                out[m] = self.levels[-1][0, 0]
            lf = np.floor(level)
            for l in range(n_levels - 1):
                m = (branch == 1) & (lf == l)
                if m.any():
                    d = (level[m] - l)[:, None]
                    out[m] = (1 - d) * self.triangle(l, st[m]) + d * self.triangle(l + 1, st[m])
        return out, branch, level

    def lookup(self, st, dst0, dst1):
        with np.errstate(all="ignore"):
            # dst0.x.abs().max(dst0.y).max(dst1.x.abs().max(dst1.y.abs())): dst0.y enters without abs, as written
            width = np.fmax(np.fmax(np.abs(dst0[:, 0]), dst0[:, 1]), np.fmax(np.abs(dst1[:, 0]), np.abs(dst1[:, 1])))
        return self.lookup_width(st, 2.0 * width)


# ---------------------------------------------------------------- Texture::evaluate and the materials
class Ref:
    """the restatement over one SceneBuilder"""

    def __init__(self, builder):
        self.tex = [dict(kind=t.kind, is_float=bool(t.is_float), value=np.array(list(t.value), np.float64), tex1=t.tex1, tex2=t.tex2, image=t.image,
                         su=float(t.su), sv=float(t.sv), du=float(t.du), dv=float(t.dv)) for t in builder.textures]
        self.mips = [Mip(tex, wrap) for tex, wrap in builder.images]
        self.materials = [dict(type=m.type, remap=bool(m.remap_roughness), a=np.array(list(m.a), np.float64), b=np.array(list(m.b), np.float64),
                               s=np.array([m.s0, m.s1, m.s2], np.float64)) for m in builder.materials]
        self.mtex = [list(s) for s in builder.material_textures] if builder.textures else None

    def largest(self, tid):
        """the largest magnitude texture `tid` can return"""
        t = self.tex[tid]
        if t["kind"] == A.FTN_TEX_CONSTANT:
            return float(np.abs(t["value"][:1] if t["is_float"] else t["value"]).max())
        if t["kind"] == A.FTN_TEX_UV:
            return 1.0
        if t["kind"] == A.FTN_TEX_CHECKERBOARD:
            return max(self.largest(t["tex1"]), self.largest(t["tex2"]))
        return self.mips[t["image"]].largest

    def evaluate(self, tid, rows, depth=0):
        """rows [n, 6] (u, v, dudx, dvdx, dudy, dvdy) -> value [n, 3], fragile [n], info dict (the discrete outcomes along the way)"""
        rows = np.asarray(rows, np.float64)
        n = rows.shape[0]
        t = self.tex[tid]
        none = np.zeros(n, bool)
        if t["kind"] == A.FTN_TEX_CONSTANT:
            v = t["value"]
            return np.tile(np.array([v[0]] * 3 if t["is_float"] else v), (n, 1)), none, {}
        with np.errstate(all="ignore"):
            st = np.stack([t["su"] * rows[:, 0] + t["du"], t["sv"] * rows[:, 1] + t["dv"]], axis=1)
            near = (np.abs(st - np.round(st)) <= ULPS_NEAR_INTEGER * np.spacing(np.abs(st).astype(np.float32)).astype(np.float64)).any(axis=1)
            if t["kind"] == A.FTN_TEX_UV:
                return np.stack([st[:, 0] - np.floor(st[:, 0]), st[:, 1] - np.floor(st[:, 1]), np.zeros(n)], axis=1), near, {}
            if t["kind"] == A.FTN_TEX_CHECKERBOARD:
                first = wrap_i32(as_i32(np.floor(st[:, 0])) + as_i32(np.floor(st[:, 1]))) % 2 == 0
                if depth >= 63:
                    return np.zeros((n, 3)), near, {}
                v1, f1, i1 = self.evaluate(t["tex1"], rows, depth + 1)
                v2, f2, i2 = self.evaluate(t["tex2"], rows, depth + 1)
                info = {"child": first}
                for k in set(i1) | set(i2):
                    if k in i1 and k in i2:
                        info[k + "'"] = np.where(first, i1[k], i2[k])
                return np.where(first[:, None], v1, v2), near | np.where(first, f1, f2), info
            dst0 = np.stack([t["su"] * rows[:, 2], t["sv"] * rows[:, 3]], axis=1)
            dst1 = np.stack([t["su"] * rows[:, 4], t["sv"] * rows[:, 5]], axis=1)
            mip = self.mips[t["image"]]
            v, branch, level = mip.lookup(st, dst0, dst1)
            fragile = (np.abs(level - (len(mip.levels) - 1)) < BLACK_TOP_LEVEL) if mip.wrap == A.FTN_WRAP_BLACK else none
            return v, fragile, {"branch": branch, "level": level}

    def is_textured(self, mat):
        return self.mtex is not None and any(s >= 0 for s in self.mtex[mat])

    def resolve(self, mat, rows):
        """-> [n, 16] as the hook lays a row out (type and remap as numbers, not bits), fragile [n]"""
        rows = np.asarray(rows, np.float64)
        n = rows.shape[0]
        m = self.materials[mat]
        out = np.zeros((n, 16))
        fragile = np.zeros(n, bool)
        out[:, 0] = 1.0 if self.is_textured(mat) else 0.0
        out[:, 1] = m["type"]
        out[:, 3:6], out[:, 6:9], out[:, 9:12] = m["a"], m["b"], m["s"]
        if self.is_textured(mat):
            ta, tb, t0, t1, t2 = self.mtex[mat]
            for tid, cols in ((ta, slice(3, 6)), (tb, slice(6, 9))):
                if tid >= 0:
                    v, f, _ = self.evaluate(tid, rows)
                    out[:, cols] = v
                    fragile |= f
            for tid, col in ((t0, 9), (t1, 10), (t2, 11)):
                if tid >= 0:
                    v, f, _ = self.evaluate(tid, rows)
                    out[:, col] = v[:, 0]
                    fragile |= f
        remap = m["remap"]
        with np.errstate(all="ignore"):
            if m["type"] == A.FTN_MAT_MATTE:                     # matte.rs: sigma.clamp(0, 90); OrenNayar::new(r, Deg(sigma)) unless 0
                sigma = np.where(np.isnan(out[:, 9]), np.nan, np.clip(out[:, 9], 0.0, 90.0))
                s2 = np.radians(sigma) ** 2
                out[:, 9] = sigma
                out[:, 10] = np.where(sigma != 0.0, 1.0 - s2 / (2.0 * (s2 + np.float64(np.float32(0.33)))), out[:, 10])
                out[:, 11] = np.where(sigma != 0.0, np.float64(np.float32(0.45)) * s2 / (s2 + np.float64(np.float32(0.09))), out[:, 11])
            elif m["type"] in (A.FTN_MAT_METAL, A.FTN_MAT_GLASS) and remap:
                out[:, 10], out[:, 11] = roughness_to_alpha(out[:, 10]), roughness_to_alpha(out[:, 11])
            elif m["type"] == A.FTN_MAT_PLASTIC and remap:
                out[:, 10] = roughness_to_alpha(out[:, 10])
        keeps = m["type"] not in (A.FTN_MAT_METAL, A.FTN_MAT_GLASS, A.FTN_MAT_PLASTIC)
        out[:, 2] = 1.0 if (remap and keeps) else 0.0          # the remap has been applied where the material has one
        return out, fragile


def roughness_to_alpha(r):
    """microfacet.rs: the polynomial in ln(max(roughness, 1e-3)), its coefficients binary32 literals"""
    c = [np.float64(np.float32(v)) for v in (1.62142, 0.819955, 0.1734, 0.0171201, 0.000640711)]
    x = np.log(np.where(np.isnan(r), 1.0e-3, np.maximum(r, np.float64(np.float32(1.0e-3)))))
    return c[0] + c[1] * x + c[2] * x * x + c[3] * x * x * x + c[4] * x * x * x * x


# ---------------------------------------------------------------- comparisons
def rel_err(got, want, floor):
    """|got - want| / max(|want|, floor); a NaN or an infinity on one side only counts as infinite, the same one on both as 0"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(all="ignore"):
        e = np.abs(got - want) / np.maximum(np.abs(want), floor)
    same = (np.isnan(got) & np.isnan(want)) | (np.isinf(got) & np.isinf(want) & (got == want))
    e = np.where(same, 0.0, e)
    return np.where(np.isnan(e), np.inf, e)
