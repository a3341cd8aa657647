"""Shared by tests/test_texture_cpu.py (the oracle) and tests/test_texture.py (the device): the texture and material configurations, the rows
fed to the hooks (ftn_test_texture_eval / orc_test_texture_eval, ftn_test_material / orc_test_material, ftn_test_mipmap_level /
orc_test_mipmap_level), the measured tolerances and the property checks, so that both sides face the same seeds and the same bounds.
DESIGN.md 3.4."""
import ctypes as C

import numpy as np

import _texture_ref as X
from _rows import run_rows
from fountain_amd import SceneBuilder, _abi as A

f32 = np.float32
U24 = 2.0 ** -24                       # half an ulp of 1: the relative rounding error of one binary32 operation
WRAPS = ("repeat", "black", "clamp")
# (h, w): 1x1 has one level (every positive width reads the top texel); 1xN / Nx1 keep one axis at a single texel through every level; 3x3, 5x4,
# 12x20, 17x33 / 33x17 halve unevenly (the taps of the pyramid are not the 2:1 box-like ones) and tell lw from lh; 1x32768 fills all 16 levels
IMAGE_SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (5, 4), (16, 16), (12, 20), (17, 33), (33, 17), (1, 32768)]
MAPPING = dict(scale=0.75, uscale=1.5, vscale=0.75, udelta=0.25, vdelta=-0.125)
N_ROWS = 100000


def shape_name(shape):
    return "%dx%d" % shape


def image(shape, seed=None):
    rng = np.random.default_rng(1000 * shape[0] + shape[1] if seed is None else seed)
    return (0.05 + 0.95 * rng.random(shape + (3,))).astype(f32)


def ramp_function(st):
    """the affine image of the ramp scene, as a function of st (row 0 of the STORED image is t = 0)"""
    st = np.asarray(st, np.float64)
    return np.stack([0.25 + 0.5 * st[:, 0] + 0.125 * st[:, 1], 0.75 - 0.25 * st[:, 0] + 0.125 * st[:, 1], 0.5 + 0.375 * st[:, 1]], axis=1)


RAMP = (32, 32)
FCHK = dict(sigma_lo=(-5.0, 0.0), sigma_hi=(45.0, 120.0), rough=(0.05, 0.4), rough2=(0.0005, 0.9), eta=(1.25, 1.75))
SAME = dict(Kd=(0.25, 0.5, 0.75), Ks=(0.5, 0.25, 0.125), sigma=33.0, rough=0.2, rough2=0.45, eta=1.5)      # the constants of the "same" scene


# ---------------------------------------------------------------- the scenes: name -> builder, {texture name: index}, {material name: index}
def build(be, name):
    b = SceneBuilder(be)
    tex, mat = {}, {}
    if name.startswith("img_"):                                   # one image shape under the three wrap modes, mapped and unmapped
        shape = tuple(int(v) for v in name[4:].split("x"))
        img = image(shape)
        for wrap in WRAPS:
            tex[wrap] = b.texture(wrap, "spectrum", "imagemap", texels=img, wrap=wrap, **MAPPING)
            tex["id_" + wrap] = b.texture("id_" + wrap, "spectrum", "imagemap", texels=img, wrap=wrap)
    elif name == "const":                                         # the constant image of every shape (mipmap.rs, test_mipmap_lookup)
        for shape in IMAGE_SHAPES:
            for wrap in ("repeat", "clamp"):
                n = shape_name(shape) + "_" + wrap
                tex[n] = b.texture(n, "spectrum", "imagemap", texels=np.full(shape + (3,), 0.5, f32), wrap=wrap, uscale=1.5, vscale=0.75, udelta=0.25, vdelta=-0.125)
    elif name == "special":
        h, w = RAMP
        centres = np.stack(np.meshgrid((np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h), axis=-1).reshape(-1, 2)
        stored = ramp_function(centres).reshape(h, w, 3)
        huge, nan = image((5, 4), 7), image((5, 4), 8)
        huge[2, 1, 1] = 1.0e30
        nan[3, 2, 0] = np.nan
        for wrap in WRAPS:
            tex["ramp_" + wrap] = b.texture("ramp_" + wrap, "spectrum", "imagemap", texels=stored[::-1], wrap=wrap)
            tex["huge_" + wrap] = b.texture("huge_" + wrap, "spectrum", "imagemap", texels=huge, wrap=wrap, **MAPPING)
            tex["nan_" + wrap] = b.texture("nan_" + wrap, "spectrum", "imagemap", texels=nan, wrap=wrap, **MAPPING)
            tex["gamma_" + wrap] = b.texture("gamma_" + wrap, "spectrum", "imagemap", texels=image((12, 20), 9), wrap=wrap, gamma=True, **MAPPING)
    elif name == "procedural":
        tex["chk"] = b.texture("chk", "spectrum", "checkerboard", uscale=8.0, vscale=4.0, udelta=0.25, tex1=(0.1, 0.2, 0.3), tex2=(0.8, 0.7, 0.6))
        tex["fchk"] = b.texture("fchk", "float", "checkerboard", uscale=3.0, vscale=5.0, vdelta=-0.5, tex1=0.0, tex2=30.0)
        tex["chk_neg"] = b.texture("chk_neg", "spectrum", "checkerboard", uscale=-3.5, vscale=-2.5, udelta=-7.25, vdelta=-11.5, tex1=(1, 2, 3), tex2=(4, 5, 6))
        tex["uv"] = b.texture("uv", "spectrum", "uv", uscale=2.0, vscale=-3.0, udelta=0.375, vdelta=0.25)
        tex["img"] = b.texture("img", "spectrum", "imagemap", texels=image((12, 20)), wrap="repeat", **MAPPING)
        tex["inner"] = b.texture("inner", "spectrum", "checkerboard", uscale=5.0, vscale=7.0, tex1="img", tex2="uv")
        tex["nest"] = b.texture("nest", "spectrum", "checkerboard", uscale=2.0, vscale=3.0, udelta=0.5, tex1="inner", tex2=(0.9, 0.8, 0.7))
    elif name in ("mats", "mats_plain"):
        if name == "mats":
            b.texture("ca", "spectrum", "checkerboard", uscale=2.0, vscale=3.0, tex1=(0.1, 0.2, 0.3), tex2=(0.8, 0.7, 0.6))
            b.texture("cb", "spectrum", "checkerboard", uscale=3.0, vscale=2.0, udelta=0.5, tex1=(1.5, 0.9, 0.2), tex2=(3.5, 2.5, 2.0))
            for i, (k, (v1, v2)) in enumerate(FCHK.items()):
                b.texture(k, "float", "checkerboard", uscale=1.0 + i, vscale=5.0 - i, udelta=0.25 * i, tex1=v1, tex2=v2)
            mat["matte_lo"] = b.material("matte", Kd="ca", sigma="sigma_lo")
            mat["matte_hi"] = b.material("matte", Kd="ca", sigma="sigma_hi")
            mat["matte_kd"] = b.material("matte", Kd="ca", sigma=120.0)
            for remap in (True, False):
                s = "_remap" if remap else "_raw"
                mat["plastic" + s] = b.material("plastic", Kd="ca", Ks="cb", roughness="rough", remaproughness=remap)
                mat["metal" + s] = b.material("metal", eta="ca", k="cb", uroughness="rough", vroughness="rough2", remaproughness=remap)
                mat["glass" + s] = b.material("glass", Kr="ca", Kt="cb", eta="eta", uroughness="rough", vroughness="rough2", remaproughness=remap)
        # materials without a textured slot: in "mats" beside textured ones, in "mats_plain" in a scene without any texture (S.mtex == NULL)
        mat["plain_matte"] = b.material("matte", Kd=(0.2, 0.4, 0.6), sigma=120.0)
        mat["plain_matte0"] = b.material("matte", Kd=(0.2, 0.4, 0.6), sigma=-3.0)
        mat["plain_plastic"] = b.material("plastic", roughness=0.3)
        mat["plain_metal"] = b.material("metal", eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.2), uroughness=0.02, vroughness=0.6, remaproughness=False)
        mat["plain_glass"] = b.material("glass", uroughness=0.1, vroughness=0.0005)
        mat["plain_mirror"] = b.material("mirror")
    elif name == "same":                                          # every slot a checkerboard whose two children hold the same constant, beside its plain twin
        for k, v in SAME.items():
            b.texture(k, "float" if np.isscalar(v) else "spectrum", "checkerboard", uscale=3.0, vscale=2.0, tex1=v, tex2=v)
        for remap in (True, False):
            s = "_remap" if remap else "_raw"
            for tw, P in (("tex_", {k: k for k in SAME}), ("plain_", SAME)):
                mat[tw + "matte" + s] = b.material("matte", Kd=P["Kd"], sigma=P["sigma"])
                mat[tw + "plastic" + s] = b.material("plastic", Kd=P["Kd"], Ks=P["Ks"], roughness=P["rough"], remaproughness=remap)
                mat[tw + "metal" + s] = b.material("metal", eta=P["Kd"], k=P["Ks"], uroughness=P["rough"], vroughness=P["rough2"], remaproughness=remap)
                mat[tw + "glass" + s] = b.material("glass", Kr=P["Kd"], Kt=P["Ks"], eta=P["eta"], uroughness=P["rough"], vroughness=P["rough2"], remaproughness=remap)
    else:
        raise KeyError(name)
    b.shape("sphere")
    return b, tex, mat


IMAGE_SCENES = ["img_" + shape_name(s) for s in IMAGE_SHAPES]
SCENES = IMAGE_SCENES + ["const", "special", "procedural", "mats", "mats_plain", "same"]


class Hook:
    """one scene on one backend, its hooks, and the restatement of the same builder"""

    def __init__(self, be, name):
        self.be, self.name = be, name
        self.builder, self.tex, self.mat = build(be, name)
        self.scene = self.builder.create_scene()
        self.ref = X.Ref(self.builder)
        pre = "orc_" if be.is_oracle else "ftn_"
        self.f_tex, self.f_mat, self.f_mip = (getattr(be.lib, pre + n) for n in ("test_texture_eval", "test_material", "test_mipmap_level"))
        self.f_tex.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
        self.f_mat.argtypes = A.TEST_MATERIAL_ARGTYPES
        self.f_mip.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        for f in (self.f_tex, self.f_mat, self.f_mip):
            f.restype = C.c_int

    def targets(self):
        """every texture and material of the scene the tests name: [("tex" | "mat", name)]"""
        return [("tex", k) for k in self.tex] + [("mat", k) for k in self.mat]

    def _run(self, fn, index, rows, width):
        return run_rows(self.be, lambda pin, n, pout: fn(self.scene.handle, index, pin, n, pout), rows, 6, width)

    def eval(self, tex, rows):
        return self._run(self.f_tex, self.tex[tex], rows, 3)

    def resolve(self, mat, rows):
        return self._run(self.f_mat, self.mat[mat], rows, A.FTN_TEST_MATERIAL_OUT)

    def run(self, target, rows):
        return self.eval(target[1], rows) if target[0] == "tex" else self.resolve(target[1], rows)

    def stored(self, tex):
        """the level-0 texels of an image texture as the builder holds them (scaled, decoded, row 0 = t 0), and its wrap mode"""
        return self.builder.images[self.builder.textures[self.tex[tex]].image]

    def levels(self, tex):
        """the backend's own pyramid of an image texture (the host builder of the product / the oracle's)"""
        img = self.stored(tex)[0]
        h, w = img.shape[:2]
        out = []
        lw, lh = C.c_uint32(), C.c_uint32()
        while self.f_mip(w, h, img.ctypes.data_as(C.c_void_p), len(out), C.cast(C.byref(lw), C.c_void_p), C.cast(C.byref(lh), C.c_void_p), None) == 0:
            lev = np.empty((lh.value, lw.value, 3), f32)
            assert self.f_mip(w, h, img.ctypes.data_as(C.c_void_p), len(out), None, None, lev.ctypes.data_as(C.c_void_p)) == 0
            out.append(lev)
        return out


# ---------------------------------------------------------------- rows
def random_rows(seed, n=N_ROWS):
    """the rows of tests/test_textures.py::test_texture_evaluate_on_device: uv in [-3, 5), differentials N(0, 1) * exp(U(-9, 1)), 2 % of them zero"""
    rng = np.random.default_rng(seed)
    rows = np.concatenate([rng.random((n, 2)) * 8 - 3, rng.standard_normal((n, 4)) * np.exp(rng.uniform(-9, 1, (n, 1)))], axis=1).astype(f32)
    rows[: n // 50, 2:] = 0.0
    return rows


def far_rows(seed, n=N_ROWS):
    """uv of 10^3 ... 10^5, either sign: binary32 loses the position inside a texel there"""
    rng = np.random.default_rng(seed)
    rows = random_rows(seed + 1, n)
    rows[:, :2] = (10.0 ** rng.uniform(3, 5, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))).astype(f32)
    return rows


def edge_rows(img_shape):
    """uv at +-0, 1, exact texel centres and edges of every level, +-1e10, +-inf, NaN and a denormal; widths 0, exact powers of two, 1 and 10, in
    each of the four differentials and with either sign.  Meant for the unmapped textures ("id_*"): st = uv there."""
    h, w = img_shape
    special = [0.0, -0.0, 1.0, 1.0e10, -1.0e10, np.inf, -np.inf, np.nan, 1.0e-40, 0.5, -0.25]

    def axis(n):
        v = list(special)
        while True:
            for k in sorted({0, 1, n // 2, n - 1, n}):
                v += [k / n, (k + 0.5) / n, (k - 0.5) / n]
            if n == 1:
                return np.unique(np.array(v, f32).view(np.uint32)).view(f32)       # by bits: keeps -0 and NaN
            n = max(1, n // 2)
    us, vs = axis(w), axis(h)
    rng = np.random.default_rng(w * 7 + h)
    if len(us) > 48:
        us = np.concatenate([np.array(special, f32), rng.choice(us, 48 - len(special), replace=False)])
    if len(vs) > 48:
        vs = np.concatenate([np.array(special, f32), rng.choice(vs, 48 - len(special), replace=False)])
    widths = [0.0] + [2.0 ** -k for k in (1, 2, 3, 5, 8, 12, 15, 16, 20)] + [1.0, 10.0, 0.3]
    diffs = []
    for wd in widths:
        for slot in range(4):
            for sign in (1.0, -1.0):
                d = [0.0] * 4
                d[slot] = sign * wd / 2.0                # lookup_trilinear doubles the largest differential
                diffs.append(d)
        diffs.append([wd / 2.0, -wd / 4.0, -wd / 2.0, wd / 8.0])
    diffs = np.unique(np.array(diffs, f32), axis=0)
    uv = np.stack(np.meshgrid(us, vs), axis=-1).reshape(-1, 2)
    pick = rng.integers(0, len(diffs), (len(uv), 6))     # six differentials per coordinate pair
    return np.concatenate([np.repeat(uv, 6, axis=0), diffs[pick.reshape(-1)]], axis=1).astype(f32)


# ---------------------------------------------------------------- layer 1: against the restatement
def floor_of(hook, target):
    """1e-3 x the largest value the rows of `target` can read (per output column for a material)"""
    if target[0] == "tex":
        return 1.0e-3 * hook.ref.largest(hook.tex[target[1]])
    return None


def errors_against_restatement(hook, target, rows):
    """-> the error of every row, the rows that are fragile; asserts the discrete outcomes of a material on the way"""
    got = hook.run(target, rows).astype(np.float64)
    if target[0] == "tex":
        want, fragile, _ = hook.ref.evaluate(hook.tex[target[1]], rows)
        return X.rel_err(got, want, floor_of(hook, target)).max(axis=1), fragile
    want, fragile = hook.ref.resolve(hook.mat[target[1]], rows)
    raw = hook.run(target, rows)
    assert np.array_equal(raw[:, 0], want[:, 0].astype(f32)) and np.array_equal(raw[:, 1:3].view(np.uint32), want[:, 1:3].astype(np.uint32)), target
    assert not raw[:, 12:].any(), target
    floor = 1.0e-3 * np.maximum(np.nanmax(np.abs(want[:, 3:12]), axis=0), 1.0e-30)
    return X.rel_err(got[:, 3:12], want[:, 3:12], floor).max(axis=1), fragile


def summary(err, fragile, select=None):
    """-> (99.9th percentile, maximum) of the error over the rows kept, the share left out"""
    if select is not None:
        err, fragile = err[select], fragile[select]
    e = err[~fragile]
    return (float(np.percentile(e, 99.9)) if e.size else 0.0), (float(e.max()) if e.size else 0.0), float(fragile.mean()) if fragile.size else 0.0


def compare_with_restatement(hook, target, rows):
    return summary(*errors_against_restatement(hook, target, rows))


def beyond_binary32(rows):
    """the rows of an edge table at uv = +-1e10: st * w is past 2^31 there, the tap index saturates, the four weights are of the size of st * w
    and cancel -- what binary32 returns is rounding noise around what binary64 returns, and only NaN against number can be told apart"""
    return (np.abs(rows[:, :2]) == f32(1.0e10)).any(axis=1)


def compare_levels(hook, tex):
    """the backend's pyramid against the restatement's: the largest |got - want| / the largest texel over all levels"""
    img = hook.stored(tex)[0]
    got, want = hook.levels(tex), X.pyramid(img)
    assert [l.shape for l in got] == [l.shape for l in want], tex
    return max(float(np.abs(g - w).max()) for g, w in zip(got, want)) / float(np.abs(img).max())


# measured with the libm oracle against the restatement (tests/test_texture_cpu.py prints the figures): (99.9th percentile, maximum) per
# configuration; the tests bound every configuration at TOL_FACTOR x its own figure (binary32 rounding of one formula differs between builds
# by small factors)
TOL_FACTOR = 4.0
# the edge table seeks the top level out (one width in thirteen is exactly 1, where the level is exactly n_levels - 1), so in `black` mode
# about 7 % of its rows fall under the rule that leaves a level within 1e-5 of n_levels - 1 out; check_top_texel covers those rows instead.
# MEASURED_EDGE_1E10: the rows at uv = +-1e10 (beyond_binary32) -- their figures say that nothing but NaN against number is checked there.
MAX_EDGE_FRAGILE_SHARE = 0.10
MEASURED = {
    "img_1x1/repeat": (1.53e-07, 1.74e-07),
    "img_1x1/id_repeat": (1.31e-07, 1.89e-07),
    "img_1x1/black": (1.94e-06, 2.61e-05),
    "img_1x1/id_black": (6.96e-07, 2.09e-05),
    "img_1x1/clamp": (1.53e-07, 1.74e-07),
    "img_1x1/id_clamp": (1.31e-07, 1.89e-07),
    "img_1x7/repeat": (1.28e-05, 2.43e-05),
    "img_1x7/id_repeat": (4.98e-06, 7.63e-06),
    "img_1x7/black": (1.75e-06, 1.99e-04),
    "img_1x7/id_black": (7.90e-07, 3.64e-05),
    "img_1x7/clamp": (6.38e-07, 2.21e-06),
    "img_1x7/id_clamp": (4.42e-07, 9.79e-07),
    "img_7x1/repeat": (3.25e-06, 6.77e-06),
    "img_7x1/id_repeat": (3.05e-06, 4.10e-06),
    "img_7x1/black": (1.50e-06, 3.11e-04),
    "img_7x1/id_black": (7.00e-07, 2.95e-05),
    "img_7x1/clamp": (6.48e-07, 1.23e-06),
    "img_7x1/id_clamp": (3.66e-07, 5.87e-07),
    "img_2x2/repeat": (2.82e-06, 4.33e-06),
    "img_2x2/id_repeat": (4.48e-07, 1.48e-06),
    "img_2x2/black": (1.50e-06, 7.28e-05),
    "img_2x2/id_black": (3.39e-07, 2.55e-05),
    "img_2x2/clamp": (2.80e-07, 6.61e-07),
    "img_2x2/id_clamp": (1.64e-07, 2.53e-07),
    "img_3x3/repeat": (5.10e-06, 1.77e-05),
    "img_3x3/id_repeat": (2.58e-06, 7.34e-06),
    "img_3x3/black": (1.65e-06, 1.03e-04),
    "img_3x3/id_black": (9.98e-07, 8.30e-05),
    "img_3x3/clamp": (6.24e-07, 1.65e-06),
    "img_3x3/id_clamp": (4.18e-07, 9.53e-07),
    "img_5x4/repeat": (3.79e-06, 8.75e-06),
    "img_5x4/id_repeat": (3.13e-06, 6.75e-06),
    "img_5x4/black": (1.21e-06, 8.07e-05),
    "img_5x4/id_black": (6.24e-07, 1.79e-05),
    "img_5x4/clamp": (8.25e-07, 2.25e-06),
    "img_5x4/id_clamp": (4.48e-07, 1.11e-06),
    "img_16x16/repeat": (1.30e-05, 2.95e-05),
    "img_16x16/id_repeat": (1.79e-06, 1.38e-05),
    "img_16x16/black": (1.40e-06, 8.35e-05),
    "img_16x16/id_black": (3.68e-07, 7.28e-06),
    "img_16x16/clamp": (1.98e-06, 6.24e-06),
    "img_16x16/id_clamp": (3.33e-07, 8.05e-07),
    "img_12x20/repeat": (2.72e-05, 9.29e-05),
    "img_12x20/id_repeat": (1.15e-05, 3.04e-05),
    "img_12x20/black": (1.84e-06, 2.25e-04),
    "img_12x20/id_black": (1.21e-06, 7.30e-05),
    "img_12x20/clamp": (2.90e-06, 1.03e-05),
    "img_12x20/id_clamp": (2.17e-06, 6.49e-06),
    "img_17x33/repeat": (3.34e-05, 9.18e-05),
    "img_17x33/id_repeat": (1.77e-05, 4.52e-05),
    "img_17x33/black": (2.08e-06, 8.34e-05),
    "img_17x33/id_black": (1.18e-06, 4.11e-05),
    "img_17x33/clamp": (3.28e-06, 1.12e-05),
    "img_17x33/id_clamp": (2.60e-06, 1.06e-05),
    "img_33x17/repeat": (2.31e-05, 6.93e-05),
    "img_33x17/id_repeat": (1.86e-05, 7.17e-05),
    "img_33x17/black": (1.98e-06, 9.88e-04),
    "img_33x17/id_black": (1.29e-06, 1.96e-05),
    "img_33x17/clamp": (4.83e-06, 1.25e-05),
    "img_33x17/id_clamp": (2.64e-06, 7.59e-06),
    "img_1x32768/repeat": (1.17e-02, 7.97e-02),
    "img_1x32768/id_repeat": (2.49e-07, 1.35e-05),
    "img_1x32768/black": (8.88e-06, 1.39e-03),
    "img_1x32768/id_black": (9.17e-07, 1.98e-05),
    "img_1x32768/clamp": (1.45e-04, 2.56e-03),
    "img_1x32768/id_clamp": (2.64e-07, 4.26e-07),
    "const/1x1_repeat": (1.19e-07, 1.19e-07),
    "const/1x1_clamp": (1.19e-07, 1.19e-07),
    "const/1x7_repeat": (1.19e-07, 1.19e-07),
    "const/1x7_clamp": (5.96e-08, 1.19e-07),
    "const/7x1_repeat": (1.19e-07, 2.38e-07),
    "const/7x1_clamp": (1.19e-07, 2.38e-07),
    "const/2x2_repeat": (5.96e-08, 1.19e-07),
    "const/2x2_clamp": (5.96e-08, 1.19e-07),
    "const/3x3_repeat": (5.96e-08, 1.19e-07),
    "const/3x3_clamp": (5.96e-08, 1.19e-07),
    "const/5x4_repeat": (1.19e-07, 1.19e-07),
    "const/5x4_clamp": (1.19e-07, 1.79e-07),
    "const/16x16_repeat": (5.96e-08, 1.19e-07),
    "const/16x16_clamp": (5.96e-08, 1.19e-07),
    "const/12x20_repeat": (1.19e-07, 1.79e-07),
    "const/12x20_clamp": (1.19e-07, 1.79e-07),
    "const/17x33_repeat": (2.38e-07, 2.38e-07),
    "const/17x33_clamp": (2.38e-07, 2.38e-07),
    "const/33x17_repeat": (2.38e-07, 2.38e-07),
    "const/33x17_clamp": (2.38e-07, 2.38e-07),
    "const/1x32768_repeat": (5.96e-08, 1.19e-07),
    "const/1x32768_clamp": (5.96e-08, 1.19e-07),
    "special/ramp_repeat": (2.05e-06, 6.37e-06),
    "special/huge_repeat": (5.20e-05, 9.03e-04),
    "special/nan_repeat": (3.00e-06, 5.66e-06),
    "special/gamma_repeat": (6.68e-05, 4.97e-04),
    "special/ramp_black": (5.45e-07, 9.66e-06),
    "special/huge_black": (4.80e-07, 1.46e-05),
    "special/nan_black": (1.41e-06, 9.37e-05),
    "special/gamma_black": (2.12e-06, 5.53e-05),
    "special/ramp_clamp": (2.51e-07, 3.45e-07),
    "special/huge_clamp": (2.59e-06, 1.69e-05),
    "special/nan_clamp": (5.73e-07, 1.65e-06),
    "special/gamma_clamp": (6.25e-06, 3.23e-05),
    "procedural/chk": (0.00e+00, 0.00e+00),
    "procedural/fchk": (0.00e+00, 0.00e+00),
    "procedural/chk_neg": (0.00e+00, 0.00e+00),
    "procedural/uv": (1.19e-04, 4.77e-04),
    "procedural/img": (2.65e-05, 6.20e-05),
    "procedural/inner": (7.82e-05, 4.77e-04),
    "procedural/nest": (4.17e-05, 4.77e-04),
    "mats/matte_lo": (0.00e+00, 0.00e+00),
    "mats/matte_hi": (9.93e-08, 9.93e-08),
    "mats/matte_kd": (7.29e-08, 7.29e-08),
    "mats/plastic_remap": (8.87e-08, 8.87e-08),
    "mats/metal_remap": (2.00e-06, 2.00e-06),
    "mats/glass_remap": (2.00e-06, 2.00e-06),
    "mats/plastic_raw": (0.00e+00, 0.00e+00),
    "mats/metal_raw": (0.00e+00, 0.00e+00),
    "mats/glass_raw": (0.00e+00, 0.00e+00),
    "mats/plain_matte": (7.29e-08, 7.29e-08),
    "mats/plain_matte0": (0.00e+00, 0.00e+00),
    "mats/plain_plastic": (5.81e-08, 5.81e-08),
    "mats/plain_metal": (0.00e+00, 0.00e+00),
    "mats/plain_glass": (2.00e-06, 2.00e-06),
    "mats/plain_mirror": (0.00e+00, 0.00e+00),
    "mats_plain/plain_matte": (7.29e-08, 7.29e-08),
    "mats_plain/plain_matte0": (0.00e+00, 0.00e+00),
    "mats_plain/plain_plastic": (5.81e-08, 5.81e-08),
    "mats_plain/plain_metal": (0.00e+00, 0.00e+00),
    "mats_plain/plain_glass": (2.00e-06, 2.00e-06),
    "mats_plain/plain_mirror": (0.00e+00, 0.00e+00),
    "same/tex_matte_remap": (7.71e-08, 7.71e-08),
    "same/tex_plastic_remap": (7.61e-08, 7.61e-08),
    "same/tex_metal_remap": (7.61e-08, 7.61e-08),
    "same/tex_glass_remap": (7.61e-08, 7.61e-08),
    "same/plain_matte_remap": (7.71e-08, 7.71e-08),
    "same/plain_plastic_remap": (7.61e-08, 7.61e-08),
    "same/plain_metal_remap": (7.61e-08, 7.61e-08),
    "same/plain_glass_remap": (7.61e-08, 7.61e-08),
    "same/tex_matte_raw": (7.71e-08, 7.71e-08),
    "same/tex_plastic_raw": (0.00e+00, 0.00e+00),
    "same/tex_metal_raw": (0.00e+00, 0.00e+00),
    "same/tex_glass_raw": (0.00e+00, 0.00e+00),
    "same/plain_matte_raw": (7.71e-08, 7.71e-08),
    "same/plain_plastic_raw": (0.00e+00, 0.00e+00),
    "same/plain_metal_raw": (0.00e+00, 0.00e+00),
    "same/plain_glass_raw": (0.00e+00, 0.00e+00),
}
MEASURED_FAR = {
    "img_12x20/repeat": (3.74e-01, 8.70e-01),
    "img_12x20/id_repeat": (1.70e-01, 4.28e-01),
    "img_12x20/black": (5.11e-08, 5.11e-08),
    "img_12x20/id_black": (1.03e-07, 1.03e-07),
    "img_12x20/clamp": (2.31e-07, 3.46e-07),
    "img_12x20/id_clamp": (2.78e-07, 3.67e-07),
    "img_17x33/repeat": (5.32e-01, 2.24e+00),
    "img_17x33/id_repeat": (2.46e-01, 5.24e-01),
    "img_17x33/black": (1.23e-07, 1.23e-07),
    "img_17x33/id_black": (1.23e-07, 1.23e-07),
    "img_17x33/clamp": (5.61e-07, 1.35e-06),
    "img_17x33/id_clamp": (5.30e-07, 1.07e-06),
}
MEASURED_EDGE = {
    "img_1x1/repeat": (0.00e+00, 0.00e+00),
    "img_1x1/black": (0.00e+00, 0.00e+00),
    "img_1x1/clamp": (0.00e+00, 0.00e+00),
    "img_1x7/repeat": (1.47e-06, 1.47e-06),
    "img_1x7/black": (2.07e-04, 2.07e-04),
    "img_1x7/clamp": (3.16e-07, 3.16e-07),
    "img_7x1/repeat": (3.04e-07, 3.04e-07),
    "img_7x1/black": (1.92e-04, 1.92e-04),
    "img_7x1/clamp": (2.88e-07, 2.88e-07),
    "img_2x2/repeat": (6.87e-08, 6.87e-08),
    "img_2x2/black": (6.87e-08, 6.87e-08),
    "img_2x2/clamp": (6.87e-08, 6.87e-08),
    "img_3x3/repeat": (1.83e-06, 1.83e-06),
    "img_3x3/black": (1.19e-04, 1.19e-04),
    "img_3x3/clamp": (7.48e-07, 7.48e-07),
    "img_5x4/repeat": (1.32e-06, 1.32e-06),
    "img_5x4/black": (1.32e-06, 1.32e-06),
    "img_5x4/clamp": (1.32e-06, 1.32e-06),
    "img_16x16/repeat": (2.16e-07, 2.55e-07),
    "img_16x16/black": (5.46e-07, 5.61e-07),
    "img_16x16/clamp": (2.22e-07, 2.45e-07),
    "img_12x20/repeat": (2.88e-06, 4.44e-06),
    "img_12x20/black": (4.38e-04, 4.63e-04),
    "img_12x20/clamp": (1.34e-06, 2.01e-06),
    "img_17x33/repeat": (4.99e-06, 4.99e-06),
    "img_17x33/black": (3.94e-04, 4.73e-04),
    "img_17x33/clamp": (2.06e-06, 3.38e-06),
    "img_33x17/repeat": (3.80e-06, 6.95e-06),
    "img_33x17/black": (4.32e-04, 4.65e-04),
    "img_33x17/clamp": (2.84e-06, 6.95e-06),
    "img_1x32768/repeat": (1.75e-07, 1.98e-07),
    "img_1x32768/black": (2.18e-07, 1.40e-06),
    "img_1x32768/clamp": (2.43e-07, 2.43e-07),
}
MEASURED_EDGE_1E10 = {
    "img_1x1/repeat": (2.47e+02, 2.47e+02),
    "img_1x1/black": (0.00e+00, 0.00e+00),
    "img_1x1/clamp": (2.47e+02, 2.47e+02),
    "img_1x7/repeat": (1.00e+00, 1.00e+00),
    "img_1x7/black": (4.84e-08, 4.84e-08),
    "img_1x7/clamp": (1.55e+03, 1.55e+03),
    "img_7x1/repeat": (5.51e+02, 5.51e+02),
    "img_7x1/black": (1.06e-07, 1.06e-07),
    "img_7x1/clamp": (4.97e+02, 5.49e+02),
    "img_2x2/repeat": (3.03e-07, 3.03e-07),
    "img_2x2/black": (6.87e-08, 6.87e-08),
    "img_2x2/clamp": (9.21e+02, 9.21e+02),
    "img_3x3/repeat": (1.36e+03, 1.36e+03),
    "img_3x3/black": (1.19e-07, 1.19e-07),
    "img_3x3/clamp": (1.59e+03, 1.59e+03),
    "img_5x4/repeat": (1.00e+00, 1.00e+00),
    "img_5x4/black": (1.23e-07, 1.23e-07),
    "img_5x4/clamp": (2.20e+03, 2.20e+03),
    "img_16x16/repeat": (7.92e-04, 4.43e-03),
    "img_16x16/black": (8.47e-08, 8.47e-08),
    "img_16x16/clamp": (1.48e+04, 1.48e+04),
    "img_12x20/repeat": (2.42e+03, 3.74e+03),
    "img_12x20/black": (1.03e-07, 1.03e-07),
    "img_12x20/clamp": (1.38e+04, 1.38e+04),
    "img_17x33/repeat": (1.00e+00, 1.00e+00),
    "img_17x33/black": (1.23e-07, 1.23e-07),
    "img_17x33/clamp": (1.81e+04, 1.81e+04),
    "img_33x17/repeat": (1.39e+04, 1.39e+04),
    "img_33x17/black": (5.27e-08, 5.27e-08),
    "img_33x17/clamp": (1.07e+04, 1.07e+04),
    "img_1x32768/repeat": (1.00e+00, 1.00e+00),
    "img_1x32768/black": (7.65e-08, 7.65e-08),
    "img_1x32768/clamp": (1.15e+07, 1.15e+07),
}
MEASURED_LEVELS = 1.47e-07


def bound(table, key):
    p, m = table[key]
    return TOL_FACTOR * p, TOL_FACTOR * m


# ---------------------------------------------------------------- layer 2: properties no reading of the reference enters
def ulps(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def image_textures(hook, prefix=""):
    return [k for k in hook.tex if hook.builder.textures[hook.tex[k]].kind == A.FTN_TEX_IMAGE and k.startswith(prefix)]


def check_constant_image(hook):
    """mipmap.rs, test_mipmap_lookup, for MIPMap::new and every shape: a constant 0.5 image reads back 0.5 within 6 ulps at every uv and width"""
    rows = random_rows(11, 20000)
    for k in hook.tex:
        assert ulps(hook.eval(k, rows), f32(0.5)).max() <= 6, k


def check_range(hook):
    """every weight of the pyramid and of the lookups is non-negative and each set sums to 1, so a value is a convex combination of level-0 texels
    (and of 0 in `black` mode).  Rounding: a pyramid texel is two normalised sums of at most 7 products, each within 8 roundings of convex, per
    level; a lookup is two 4-term sums and a lerp, 12 roundings."""
    rows = random_rows(12, 20000)
    for k in image_textures(hook):
        img, wrap = hook.stored(k)
        lo, hi = float(img.min()), float(img.max())
        if wrap == A.FTN_WRAP_BLACK:
            lo = min(lo, 0.0)
        n_levels = 1 + int(np.floor(np.log2(max(img.shape[:2]))))
        slack = (16 * n_levels + 12) * U24 * max(abs(lo), abs(hi))
        v = hook.eval(k, rows).astype(np.float64)
        assert v.min() >= lo - slack and v.max() <= hi + slack, (k, v.min() - lo, v.max() - hi)


def check_ramp(hook):
    """an affine image comes back as the same affine function of st at every width, as long as no tap of the levels used reaches the border
    texel of its level: levels up to 3 are used, st within [1.5 / w_l, 1 - 1.5 / w_l] of the coarser level used (0.5 / w at level 0).  Pins the -0.5 offsets of the
    lookup and of the pyramid and the alignment between levels.  Rounding: values <= 1.25, at most 3 pyramid levels of 16 roundings each and 12 of
    the lookup: 60 half-ulps of 1.25, and the position st * w_l rounds to half an ulp of 32 times the slope (< 1 per unit st)."""
    rng = np.random.default_rng(13)
    n = 20000
    n_levels = 6
    level = rng.uniform(-2.0, 3.0, n)
    level[: n // 4] = rng.integers(0, 3, n // 4)                                  # exact powers of two as well
    width = np.where(level <= -1.5, 0.0, 2.0 ** (level - (n_levels - 1)))
    coarse = np.where(level < 0, 0, np.floor(level) + 1)
    wl = RAMP[1] / 2.0 ** coarse
    margin = np.where(level < 0, 0.5, 1.5) / wl
    st = margin[:, None] + rng.random((n, 2)) * (1 - 2 * margin[:, None])
    rows = np.zeros((n, 6), f32)
    rows[:, :2] = st
    rows[:, 2] = width / 2
    rows[::2, 2] *= -1
    rows[1::4, 4], rows[1::4, 2] = rows[1::4, 2], 0.0                             # through dudy as well
    want = ramp_function(rows[:, :2])
    for wrap in WRAPS:
        got = hook.eval("ramp_" + wrap, rows)
        err = np.abs(got - want).max()
        assert err <= 60 * U24 * 1.25 + 32 * U24, (wrap, err)


def check_periodic(hook):
    """`repeat` is periodic in st.  st on a grid of 2^-12 and a shift k <= 4 are exact in binary32; st * w then rounds to half an ulp of
    (1 + k) * w, which moves the taps by that many texels: the value moves by at most the texel range times that, per axis, plus the 12
    roundings of the lookup"""
    rng = np.random.default_rng(14)
    n = 20000
    rows = random_rows(15, n)
    rows[:, :2] = rng.integers(0, 4096, (n, 2)) / 4096.0
    k = rng.integers(-4, 5, (n, 2))
    moved = rows.copy()
    moved[:, :2] += k
    img, _ = hook.stored("id_repeat")
    h, w = img.shape[:2]
    tol = 2 * float(img.max() - img.min()) * float(np.spacing(f32(5 * max(w, h)))) + 12 * U24 * float(img.max())
    d = np.abs(hook.eval("id_repeat", rows).astype(np.float64) - hook.eval("id_repeat", moved)).max()
    assert d <= tol, (d, tol)


def check_outside(hook):
    """zero footprint, st more than a texel outside [0, 1] on both axes: `black` is exactly 0, `clamp` is the corner texel (four equal taps
    whose weights sum to 1 within 4 roundings)"""
    img, _ = hook.stored("id_black")
    h, w = img.shape[:2]
    rng = np.random.default_rng(16)
    n = 4000
    side = rng.integers(0, 2, (n, 2))
    out = (1.0 / np.array([w, h]) + rng.random((n, 2)) * 3 + 1.0e-3)
    rows = np.zeros((n, 6), f32)
    rows[:, :2] = np.where(side == 0, -out, 1 + out)
    assert not hook.eval("id_black", rows).any()
    corner = img[np.where(side[:, 1] == 0, 0, h - 1), np.where(side[:, 0] == 0, 0, w - 1)]
    assert ulps(hook.eval("id_clamp", rows), corner).max() <= 4
    one = rows.copy()                                     # black with ONE axis outside is 0 as well
    one[:, 1] = 0.5
    assert not hook.eval("id_black", one).any()


def check_top_texel(hook):
    """a width >= 1 returns the bits of the top texel whatever st is"""
    rows = edge_rows(hook.stored("id_repeat")[0].shape[:2])
    rows[:, 2:] = 0.0
    rows[:, 2] = np.tile(np.array([0.5, 0.75, 5.0, -0.5, 1.0e30, np.inf], f32), len(rows) // 6 + 1)[: len(rows)]
    for wrap in WRAPS:
        top = hook.levels("id_" + wrap)[-1][0, 0]
        got = hook.eval("id_" + wrap, rows)
        assert np.array_equal(got.view(np.uint32), np.broadcast_to(top.view(np.uint32), got.shape)), wrap


def bilinear(level, wrap, st):
    """binary64, from a level's texels; st inside (0, 1)"""
    h, w = level.shape[:2]
    s, t = st[:, 0] * w - 0.5, st[:, 1] * h - 0.5
    s0, t0 = np.floor(s).astype(int), np.floor(t).astype(int)
    ds, dt = (s - s0)[:, None], (t - t0)[:, None]

    def tx(x, y):
        if wrap == A.FTN_WRAP_REPEAT:
            return level[y % h, x % w]
        v = level[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        return v if wrap == A.FTN_WRAP_CLAMP else np.where(inside[:, None], v, 0.0)
    return tx(s0, t0) * (1 - ds) * (1 - dt) + tx(s0, t0 + 1) * (1 - ds) * dt + tx(s0 + 1, t0) * ds * (1 - dt) + tx(s0 + 1, t0 + 1) * ds * dt


def check_integer_levels(hook):
    """a width of 2^-k puts the level on the integer n_levels - 1 - k: the value is that level's own bilinear read.  Bound: the 12 roundings of the
    lookup, the position (half an ulp of st * w, times the texel range per texel), and one ulp of the level (2^-19 for levels < 16) times the range
    should log2 of a power of two not be exact"""
    rng = np.random.default_rng(17)
    for wrap in WRAPS:
        levels = [l.astype(np.float64) for l in hook.levels("id_" + wrap)]
        img, wmode = hook.stored("id_" + wrap)
        rng_ = float(img.max() - min(img.min(), 0.0))
        for k in range(1, len(levels)):
            rows = np.zeros((500, 6), f32)
            rows[:, :2] = rng.random((500, 2))
            rows[:, 2 + k % 4] = 2.0 ** -k / 2
            want = bilinear(levels[len(levels) - 1 - k], wmode, rows[:, :2].astype(np.float64))
            tol = 12 * U24 * float(img.max()) + rng_ * (2 * float(np.spacing(f32(max(img.shape[:2])))) + 2.0 ** -19)
            err = np.abs(hook.eval("id_" + wrap, rows) - want).max()
            assert err <= tol, (wrap, k, err, tol)


def check_continuity_in_width(hook):
    """the value is continuous in the width across integer levels: between two widths a factor (1 + e) apart the level moves by log2(1 + e), and
    the value by at most that times the texel range (each lerp weight moves by it, each pair of levels differs by at most the range), plus two
    lookups' roundings and two ulps of the level"""
    rng = np.random.default_rng(18)
    for wrap in ("repeat", "clamp"):                      # `black` has its own discontinuity at the top level
        img, _ = hook.stored("id_" + wrap)
        n_levels = len(hook.levels("id_" + wrap))
        rng_ = float(img.max() - img.min())
        for k in range(0, n_levels):
            e = 1.0e-4
            rows = np.zeros((400, 6), f32)
            rows[:, :2] = rng.random((400, 2)) * 3 - 1
            lo, hi = rows.copy(), rows.copy()
            lo[:, 2], hi[:, 2] = 2.0 ** -k / 2 * (1 - e), 2.0 ** -k / 2 * (1 + e)
            step = np.log2(float(hi[0, 2]) / float(lo[0, 2]))
            d = np.abs(hook.eval("id_" + wrap, lo).astype(np.float64) - hook.eval("id_" + wrap, hi)).max()
            tol = (step + 2.0 ** -18) * rng_ + 24 * U24 * float(img.max())
            assert d <= tol, (wrap, k, d, tol)


def check_quirk_dst0_y(hook):
    """lookup_trilinear takes dst0.y without abs: dvdx = -0.5 alone leaves the footprint at zero, dvdx = +0.5 blurs (here: to the top texel)"""
    rows = random_rows(19, 2000)
    rows[:, 2:] = 0.0
    neg, pos, ref = rows.copy(), rows.copy(), rows.copy()
    neg[:, 3], pos[:, 3], ref[:, 2] = -0.5, 0.5, 0.5
    for wrap in WRAPS:
        k = "id_" + wrap
        sharp, blurred = hook.eval(k, rows), hook.eval(k, ref)
        assert np.array_equal(hook.eval(k, neg).view(np.uint32), sharp.view(np.uint32)), wrap
        assert np.array_equal(hook.eval(k, pos).view(np.uint32), blurred.view(np.uint32)), wrap
        if len(hook.levels(k)) > 1 and wrap != "black":
            assert (sharp != blurred).any(), wrap
        for slot in (2, 4, 5):                            # the other three differentials blur with either sign
            other = rows.copy()
            other[:, slot] = -0.5
            assert np.array_equal(hook.eval(k, other).view(np.uint32), blurred.view(np.uint32)), (wrap, slot)


def check_float_checkerboard(hook):
    v = hook.eval("fchk", random_rows(20, 20000))
    assert np.isin(v[:, 0], [0.0, 30.0]).all() and np.array_equal(v[:, 0], v[:, 1]) and np.array_equal(v[:, 0], v[:, 2])
    assert 0.4 < (v[:, 0] == 0.0).mean() < 0.6


def check_finite(hook):
    rows = np.concatenate([random_rows(21, 20000), far_rows(22, 5000)])
    for target in hook.targets():
        if target[1].startswith(("nan_", "huge_")):
            continue
        assert np.isfinite(hook.run(target, rows)).all(), target
    for wrap in WRAPS:                                    # 1e30: finite in, finite out (1e30 * weights <= 1 cannot overflow)
        if "huge_" + wrap in hook.tex:
            assert np.isfinite(hook.eval("huge_" + wrap, rows)).all()


# ---- materials
def check_same_constant(hook):
    """a material resolved per hit from checkerboards whose two children hold the same constant equals, bit for bit, the same material finalised
    at upload from those constants (the path DESIGN.md 3.1 covers)"""
    rows = random_rows(23, 5000)
    for k in hook.mat:
        if k.startswith("tex_"):
            a, b = hook.resolve(k, rows), hook.resolve("plain_" + k[4:], rows)
            assert (a[:, 0] == 1.0).all() and (b[:, 0] == 0.0).all(), k
            assert np.array_equal(a[:, 1:].view(np.uint32), b[:, 1:].view(np.uint32)), k


def oren_nayar(sigma_deg):
    s2 = np.radians(np.asarray(sigma_deg, np.float64)) ** 2
    return 1.0 - s2 / (2.0 * (s2 + 0.33)), 0.45 * s2 / (s2 + 0.09)


def check_finalising(hook):
    """sigma is clamped to [0, 90]; s1, s2 are the Oren-Nayar A, B within rounding (six binary32 operations each and the constants' own
    rounding: 8 half-ulps); a sigma of 0 leaves them untouched; with remap off, roughness passes through; remap_roughness is 0 afterwards"""
    rows = random_rows(24, 20000)
    for k, values in (("matte_lo", FCHK["sigma_lo"]), ("matte_hi", FCHK["sigma_hi"])):
        o = hook.resolve(k, rows)
        clamped = np.clip(np.array(values, f32), 0.0, 90.0)
        assert set(np.unique(o[:, 9])) == set(clamped.tolist()), (k, np.unique(o[:, 9]))
        A_, B_ = oren_nayar(o[:, 9])
        nz = o[:, 9] != 0.0
        assert np.abs(o[nz, 10] - A_[nz]).max(initial=0.0) <= 8 * U24 and np.abs(o[nz, 11] - B_[nz]).max(initial=0.0) <= 8 * U24, k
        assert not o[~nz, 10:12].any(), k                  # untouched: the builder's zeros
        assert np.isin(o[:, 3], f32([0.1, 0.8])).all()
    o = hook.resolve("matte_kd", rows)                      # a constant sigma of a textured material is finalised per hit too
    assert (o[:, 9] == 90.0).all() and (o[:, 0] == 1.0).all()
    for m in ("plastic", "metal", "glass"):
        raw, rem = hook.resolve(m + "_raw", rows), hook.resolve(m + "_remap", rows)
        assert not raw[:, 2].view(np.uint32).any() and not rem[:, 2].view(np.uint32).any(), m
        assert np.isin(raw[:, 10], f32(FCHK["rough"])).all(), m
        assert np.array_equal(raw[:, 3:10], rem[:, 3:10]), m
        want = X.roughness_to_alpha(raw[:, 10].astype(np.float64))
        # the polynomial: five terms of magnitude <= 2.7 (x = ln 5e-4 ... 0), 14 operations, and ln itself to an ulp of |x| <= 7.6
        assert np.abs(rem[:, 10] - want).max() <= 2.7 * 14 * U24 * 2 + 7.6 * 2 * U24 * 1.0, m
        if m == "plastic":
            assert not raw[:, 11].any() and not rem[:, 11].any()
        else:
            assert np.isin(raw[:, 11], f32(FCHK["rough2"])).all(), m
            assert np.abs(rem[:, 11] - X.roughness_to_alpha(raw[:, 11].astype(np.float64))).max() <= 2.7 * 14 * U24 * 2 + 7.6 * 2 * U24, m
        if m == "glass":
            assert np.isin(raw[:, 9], f32(FCHK["eta"])).all()


def check_untextured(hook, plain_hook=None):
    """an untextured material comes back as uploaded: the same in every row, the builder's record with the constant part applied"""
    rows = random_rows(25, 3000)
    for k in hook.mat:
        if not k.startswith("plain_"):
            continue
        o = hook.resolve(k, rows)
        assert (o[:, 0] == 0.0).all() and (o.view(np.uint32) == o[0].view(np.uint32)).all(), k
        m = hook.builder.materials[hook.mat[k]]
        assert o[0, 1:2].view(np.uint32)[0] == m.type and np.array_equal(o[0, 3:9], f32(list(m.a) + list(m.b))), k
        if plain_hook is not None:
            assert np.array_equal(o.view(np.uint32), plain_hook.resolve(k, rows).view(np.uint32)), k
    o = hook.resolve("plain_matte", rows)[0]
    assert o[9] == 90.0 and abs(o[10] - oren_nayar(90.0)[0]) <= 8 * U24
    o = hook.resolve("plain_matte0", rows)[0]
    assert o[9] == 0.0 and o[10] == 0.0 and o[11] == 0.0
    o = hook.resolve("plain_metal", rows)[0]
    assert o[10] == f32(0.02) and o[11] == f32(0.6) and o[2:3].view(np.uint32)[0] == 0


def check_refusals(be, hook):
    pre = "orc_" if be.is_oracle else "ftn_"
    fn = getattr(be.lib, pre + "test_material")
    fn.argtypes, fn.restype = A.TEST_MATERIAL_ARGTYPES, C.c_int
    rows, out = np.zeros((1, 6), f32), np.full((1, 16), 7.0, f32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n_mat = len(hook.builder.materials)
    assert fn(None, 0, p(rows), 1, p(out)) == A.FTN_ERR_INVALID_ARGUMENT
    assert fn(hook.scene.handle, 0, None, 1, p(out)) == A.FTN_ERR_INVALID_ARGUMENT
    assert fn(hook.scene.handle, 0, p(rows), 1, None) == A.FTN_ERR_INVALID_ARGUMENT
    assert fn(hook.scene.handle, -1, p(rows), 1, p(out)) == A.FTN_ERR_INVALID_ARGUMENT
    assert fn(hook.scene.handle, n_mat, p(rows), 1, p(out)) == A.FTN_ERR_INVALID_ARGUMENT
    assert fn(hook.scene.handle, 0, p(rows), 0, p(out)) == 0 and (out == 7.0).all()          # n == 0 does nothing
    assert fn(hook.scene.handle, n_mat - 1, p(rows), 1, p(out)) == 0 and out[0, 12:].tolist() == [0.0] * 4
