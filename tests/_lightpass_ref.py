"""A replay of the light-group pass (include/fountain_hip_lightpass.h) sample by sample, numpy restatements of its term, its shadow ray,
ftn_lightpass_resolve and ftn_lightpass_compose, and the scenes of test_lightpass.py and test_lightpass_cpu.py.

replay(): first surfaces from _ao_ref.first_surfaces (the oracle's camera rays and intersections), the light sample from the oracle's
light hook (orc_test_light), the term and the shadow ray from ftn_lightpass_terms (the kernel's code compiled for the host, pinned against
the restatements here by test_lightpass_cpu.py), occlusion from the oracle's intersect_test, and the film rule: a pixel's own samples in
increasing sample index into what the buffer holds, the samples of other pixels summed apart and added after."""
import ctypes as C

import numpy as np

from fountain_amd import _abi as A
from fountain_amd import lightpass as LP

import _ao_ref as AR
import _gbuffer_ref as GR

F32 = np.float32
bits = GR.bits
Y = np.array([0.212671, 0.715160, 0.072169], F32)
INV_PI = F32(0.318309886183790671537767526745028724)
T_MAX = F32(F32(1.0) - F32(0.0001))


# ------------------------------------------------------------------ the header's arithmetic, restated in float32
def _dot(a, b):
    return F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))


def select(u5, n):
    """k = f2usize(min(u5 * n, n - 1)) in float32"""
    return int(min(F32(F32(u5) * F32(n)), F32(n - 1)))


def term_ref(fu, lrow, n):
    """(e [3] float32, traced) of one interaction record and one light-hook row for a group of n lights"""
    fu, lrow = np.asarray(fu, F32), np.asarray(lrow, F32)
    ng, wo, ns = fu[6:9], fu[11:14], fu[20:23]
    rad, wi, pdf = lrow[0:3], lrow[3:6], lrow[6]
    zero = np.zeros(3, F32)
    if not pdf > 0 or not rad.any():
        return zero, False
    if not F32(_dot(wi, ng) * _dot(wo, ng)) > 0:
        return zero, False
    with np.errstate(all="ignore"):
        c = F32(np.abs(_dot(wi, ns)) / pdf)
        e = ((rad * c).astype(F32) * F32(n)).astype(F32)
    if not e.any():
        return zero, False
    return e, True


def ray_ref(orc, fu, lrow):
    """the shadow ray {o, d, 1 - 0.0001, 0}: both ends offset by the oracle's spawn-ray arithmetic (orc_kat_spawn_ray's origin)"""
    fu, lrow = np.asarray(fu, F32), np.asarray(lrow, F32)
    v3 = lambda a: (C.c_float * 3)(*a)
    out = (C.c_float * 8)()
    p, tp = fu[0:3], lrow[7:10]
    orc.lib.orc_kat_spawn_ray(v3(p), v3(fu[3:6]), v3(fu[6:9]), v3((tp - p).astype(F32)), out)
    origin = np.array(out[0:3], F32)
    orc.lib.orc_kat_spawn_ray(v3(tp), v3(lrow[10:13]), v3(lrow[13:16]), v3((origin - tp).astype(F32)), out)
    target = np.array(out[0:3], F32)
    return np.concatenate([origin, (target - origin).astype(F32), [T_MAX, F32(0.0)]]).astype(F32)


def luminance(c):
    c = np.asarray(c, F32)
    return F32(F32(F32(c[0] * Y[0]) + F32(c[1] * Y[1])) + F32(c[2] * Y[2]))


def resolve_ref(raw, dtype=F32):
    """ftn_lightpass_resolve in `dtype` (float32: the statement itself; float64: what it approximates)"""
    raw = np.asarray(raw, F32).reshape(-1, 8).astype(dtype)
    out = np.zeros((len(raw), 8), dtype)
    yw = Y.astype(dtype)
    for i, r in enumerate(raw):
        h, w = r[6], r[7]
        if w == 0:
            continue
        if h == 0:
            out[i, 6] = 1.0
        else:
            out[i, 0:6] = r[0:6] / h
            yl = dtype(dtype(dtype(r[0] * yw[0]) + dtype(r[1] * yw[1])) + dtype(r[2] * yw[2]))
            yu = dtype(dtype(dtype(r[3] * yw[0]) + dtype(r[4] * yw[1])) + dtype(r[5] * yw[2]))
            out[i, 6] = 1.0 if yu == 0 else yl / yu
        out[i, 7] = h / w
    return out


def compose_ref(gb12, res8, gains):
    """ftn_lightpass_compose in float32: from +0, in increasing g, ((albedo * INV_PI) * lit) * gain"""
    gb12, res8, gains = np.asarray(gb12, F32), np.asarray(res8, F32), np.asarray(gains, F32)
    acc = np.zeros(gb12.shape[:-1] + (3,), F32)
    a = (gb12[..., 0:3] * INV_PI).astype(F32)
    for g in range(res8.shape[0]):
        acc = (acc + ((a * res8[g, ..., 0:3]).astype(F32) * gains[g]).astype(F32)).astype(F32)
    acc[gb12[..., 10] == 0] = 0.0
    return acc


def synthetic_sums():
    """hand-made sums: weight == 0 (with stale values), hit_weight == 0, Y(unshadowed) == 0, fully shadowed, ordinary pixels"""
    rows = [
        [1, 2, 3, 4, 5, 6, 2, 0],                        # weight == 0: eight zeros
        [0, 0, 0, 0, 0, 0, 0, 5],                        # only misses: zero irradiance, visibility 1, coverage 0
        [0, 0, 0, 0, 0, 0, 3, 4],                        # surfaces no light reaches: Y(unshadowed) == 0, visibility 1
        [0, 0, 0, 1.5, 2.5, 0.5, 2, 2],                  # fully shadowed: visibility 0
        [1.5, 2.5, 0.5, 1.5, 2.5, 0.5, 2, 2],            # open: visibility 1
        [0.3, 0.2, 0.1, 0.9, 0.7, 0.4, 3, 7],
        [1e-30, 0, 0, 1e-30, 0, 0, 1, 1],                # luminances that underflow
    ]
    rng = np.random.default_rng(5)
    un = rng.random((64, 3)) * 4
    more = np.concatenate([un * rng.random((64, 1)), un, rng.integers(1, 10, (64, 1)), rng.integers(10, 20, (64, 1))], axis=1)
    return np.concatenate([np.array(rows, np.float64), more]).astype(F32)


# ------------------------------------------------------------------ the oracle's light samples
def draws(orc, seed, px, py, s, n=8):
    d = (C.c_float * n)()
    orc.lib.orc_kat_indexed_f32(C.c_uint64(seed), C.c_int32(px), C.c_int32(py), C.c_uint32(s), d, C.c_size_t(n))
    return np.array(d[:], F32)


def light_rows(orc, scene, light, full, u2):
    """orc_test_light's 24-float rows for the reference points of the interaction records `full` and the draws u2"""
    full, u2 = np.asarray(full, F32).reshape(-1, 24), np.asarray(u2, F32).reshape(-1, 2)
    rows = np.zeros((len(full), A.FTN_TEST_LIGHT_IN), F32)
    rows[:, 0:9], rows[:, 10:13], rows[:, 13:15] = full[:, 0:9], (0.0, 0.0, 1.0), u2
    out = np.zeros((len(full), A.FTN_TEST_LIGHT_OUT), F32)
    fn = orc.lib.orc_test_light
    fn.argtypes, fn.restype = A.TEST_LIGHT_ARGTYPES, C.c_int
    if len(full):
        orc.check(fn(scene.handle, int(light), 0, rows.ctypes.data_as(C.c_void_p), len(rows), out.ctypes.data_as(C.c_void_p)))
    return out


# ------------------------------------------------------------------ the replay
def trace(orc, ftn, make, spp, seed, lights=None, crop=(0.0, 0.0, 1.0, 1.0), tiles=None, radius=(0.5, 0.5), first_sample=0, sample_count=0):
    """every camera sample's surface, light sample, term, shadow ray and occlusion.  Returns a dict: fs (first surfaces), e [n, 3],
    rays [n, 8], traced [n], occ [n], light [n] (the chosen light's index, -1 without a surface), n_group"""
    fs = AR.first_surfaces(orc, make, spp, seed, crop, tiles, radius, first_sample, sample_count)
    sc = fs["scene"]
    M = list(range(sc.info()["n_lights"])) if lights is None else [int(i) for i in lights]
    n, N = len(M), len(fs["samples"])
    e, rays, light = np.zeros((N, 3), F32), np.zeros((N, 8), F32), np.full(N, -1, np.int64)
    hit_idx = np.array([i for i in range(N) if fs["prim"][i] >= 0], np.int64)
    if n and len(hit_idx):
        u = np.zeros((N, 2), F32)
        for i in hit_idx:
            px, py, s, _, _ = fs["samples"][i]
            d = draws(orc, seed, px, py, s)
            light[i], u[i] = M[select(d[5], n)], d[6:8]
        l24 = np.zeros((N, 24), F32)
        for li in sorted(set(light[hit_idx].tolist())):
            sel = hit_idx[light[hit_idx] == li]
            l24[sel] = light_rows(orc, sc, li, fs["full"][sel], u[sel])
        e[hit_idx], rays[hit_idx] = LP.terms(ftn, fs["full"][hit_idx], l24[hit_idx], n)
    traced = rays[:, 6] != 0
    occ = np.zeros(N, bool)
    if traced.any():
        occ[traced] = sc.intersect_test(rays[traced], stats=False)[0]
    return dict(fs=fs, e=e, rays=rays, traced=traced, occ=occ, light=light, n_group=n, hit=fs["prim"] >= 0)


def sums(tr, start=None):
    """The sums ftn_render_lightpass adds for a trace, into `start` (zeros when None).  Returns a dict: acc [H, W, 8]; foreign [H, W]
    (how many samples of other pixels the pixel received: the device adds those through the spill sums, in no fixed order when there is
    more than one); n (camera samples), n_spill, rays_closest, rays_any, hits, occluded."""
    fs = tr["fs"]
    f = fs["film"]
    c = f.desc.crop
    acc = np.zeros((f.height, f.width, 8), F32) if start is None else np.array(start, F32)
    spill = np.zeros((f.height, f.width, 8), F32)
    foreign = np.zeros((f.height, f.width), np.int64)
    n_spill = 0
    for i, (px, py, s, s5, tpb) in enumerate(fs["samples"]):
        touched = GR.footprint(f, tpb, s5[0], s5[1])
        if len(touched) != 1:
            n_spill += 1
        for (x, y) in touched:
            own = (x, y) == (px, py)
            a = (acc if own else spill)[y - c[1], x - c[0]]
            if tr["hit"][i]:
                v = (tr["e"][i] * F32(1.0)).astype(F32)
                if tr["traced"][i] and not tr["occ"][i]:
                    a[0:3] += v
                a[3:6] += v
                a[6] += F32(1.0)
            a[7] += F32(1.0)
            if not own:
                foreign[y - c[1], x - c[0]] += 1
    acc += spill
    return dict(acc=acc, foreign=foreign, n=len(fs["samples"]), n_spill=n_spill, rays_closest=fs["rays"], rays_any=int(tr["traced"].sum()),
                hits=int(tr["hit"].sum()), occluded=int(tr["occ"].sum()))


def replay(orc, ftn, make, spp, seed, lights=None, start=None, **kw):
    return sums(trace(orc, ftn, make, spp, seed, lights, **kw), start)


def assert_matches(raw, ref, what="", rtol=2e-6, atol=1e-6):
    """hit_weight and weight bit-equal on every pixel; lit and unshadowed bit-equal where at most one sample of another pixel landed (one
    spill sample is added exactly as the replay adds it) and within the tolerance of the film's reordered spill sums
    (tests/test_gbuffer.py's) where several did"""
    want = ref["acc"]
    for k, name in ((6, "hit_weight"), (7, "weight")):
        assert np.array_equal(bits(raw[..., k]), bits(want[..., k])), "%s: %s differs at %d pixels" % (what, name, int((raw[..., k] != want[..., k]).sum()))
    diff = (bits(raw[..., 0:6]) != bits(want[..., 0:6])).any(-1)
    bad = diff & (ref["foreign"] <= 1)
    assert not bad.any(), "%s: lit / unshadowed differ at %d pixels outside reordered spill pixels, first %r: %r vs %r" % (
        what, int(bad.sum()), tuple(np.argwhere(bad)[0]), raw[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])
    assert np.allclose(raw[..., 0:6], want[..., 0:6], rtol=rtol, atol=atol), "%s: beyond the spill tolerance" % what


# ------------------------------------------------------------------ scenes
def _cam(be, eye, at, up, res, fov=40.0):
    from fountain_amd import PerspectiveCamera
    return PerspectiveCamera.look_at(be, eye, at, up, res, fov=fov)


def floor_blocker(be, res=(40, 24)):
    """a floor under a point light with a floating blocker between them: part of the floor is in its shadow, the blocker's top is lit"""
    from fountain_amd import SceneBuilder, scenes
    b = SceneBuilder(be)
    b.light_source("point", I=(20, 18, 15), from_=(0.3, 0.2, 4))
    b.material("matte", Kd=(0.5, 0.5, 0.5))
    scenes._quad(b, (-6, -6, 0), (6, -6, 0), (6, 6, 0), (-6, 6, 0))
    b.material("matte", Kd=(0.7, 0.3, 0.2))
    scenes._quad(b, (-0.8, -0.6, 1.5), (0.8, -0.6, 1.5), (0.8, 0.6, 1.5), (-0.8, 0.6, 1.5))
    return b, _cam(be, (0, -7, 5), (0, 0, 0.5), (0, 0, 1), res), res


def open_floor(be, res=(24, 16)):
    """nothing stands between the floor and its two lights"""
    from fountain_amd import SceneBuilder, scenes
    b = SceneBuilder(be)
    b.light_source("point", I=(20, 18, 15), from_=(0.3, 0.2, 4))
    b.light_source("distant", L=(2, 2.5, 3), from_=(1, -1, 2), to=(0, 0, 0))
    b.material("matte", Kd=(0.5, 0.5, 0.5))
    scenes._quad(b, (-50, -50, 0), (50, -50, 0), (50, 50, 0), (-50, 50, 0))
    return b, _cam(be, (0, -3, 4), (0, 0, 0), (0, 0, 1), res), res


def covered_floor(be, res=(24, 16)):
    """a floor under a point light, with a plate far wider than the view between them: every shadow ray is stopped"""
    from fountain_amd import SceneBuilder, scenes
    b = SceneBuilder(be)
    b.light_source("point", I=(20, 18, 15), from_=(0, 0, 40))
    b.material("matte", Kd=(0.5, 0.5, 0.5))
    scenes._quad(b, (-5, -5, 0), (5, -5, 0), (5, 5, 0), (-5, 5, 0))
    scenes._quad(b, (-500, -500, 30), (500, -500, 30), (500, 500, 30), (-500, 500, 30))
    return b, _cam(be, (0, -3, 4), (0, 0, 0), (0, 0, 1), res), res


def null_quad(be, res=(40, 24)):
    """a block on a floor behind a null-material quad: the camera rays pass through the quad, which still stops shadow rays"""
    from fountain_amd import SceneBuilder, scenes
    b = SceneBuilder(be)
    b.light_source("point", I=(30, 30, 30), from_=(0, -4, 5))
    q = scenes._quad
    b.material("matte", Kd=(0.6, 0.6, 0.6))
    q(b, (-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0))
    b.material("matte", Kd=(0.7, 0.3, 0.2))
    q(b, (-0.5, -0.5, 0.8), (0.5, -0.5, 0.8), (0.5, 0.5, 0.8), (-0.5, 0.5, 0.8))
    q(b, (-0.5, -0.5, 0.0), (0.5, -0.5, 0.0), (0.5, -0.5, 0.8), (-0.5, -0.5, 0.8))
    b.material("none")
    q(b, (-1.0, -1.5, 0.0), (1.0, -1.5, 0.0), (1.0, -1.5, 2.5), (-1.0, -1.5, 2.5))
    return b, _cam(be, (0.3, -5.0, 2.2), (0.0, 0.0, 0.5), (0, 0, 1), res), res


def every_kind(be, res=(40, 24)):
    """one light of every kind -- point (0), distant (1), infinite (2), and the two triangles of an emissive quad (3, 4) -- over a floor,
    a block and a sphere"""
    from fountain_amd import SceneBuilder, scenes
    b = SceneBuilder(be)
    b.light_source("point", I=(12, 10, 8), from_=(-1.5, -1.0, 3))
    b.light_source("distant", L=(1.5, 1.5, 2.0), from_=(2, -1, 3), to=(0, 0, 0))
    b.light_source("infinite", L=(0.4, 0.5, 0.6))
    q = scenes._quad
    b.material("matte", Kd=(0.6, 0.6, 0.6))
    q(b, (-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0))
    b.material("matte", Kd=(0.2, 0.5, 0.7))
    q(b, (-1.2, -0.5, 0.9), (-0.2, -0.5, 0.9), (-0.2, 0.5, 0.9), (-1.2, 0.5, 0.9))
    q(b, (-1.2, -0.5, 0.0), (-0.2, -0.5, 0.0), (-0.2, -0.5, 0.9), (-1.2, -0.5, 0.9))
    b.attribute_begin()
    b.translate((1.0, 0.2, 0.6))
    b.shape("sphere", radius=0.6)
    b.attribute_end()
    b.attribute_begin()
    b.area_light_source("diffuse", L=(8.0, 8.0, 8.0))
    q(b, (-0.5, -0.5, 2.8), (-0.5, 0.5, 2.8), (0.5, 0.5, 2.8), (0.5, -0.5, 2.8))            # clockwise from above: faces -z
    b.attribute_end()
    return b, _cam(be, (0.3, -6.0, 3.0), (0.0, 0.0, 0.5), (0, 0, 1), res), res


def point_and_distant(be, res=(24, 16), point=True):
    """a floor and a blocker under a distant light, with (point = True: lights [point, distant]) or without a point light in front"""
    from fountain_amd import SceneBuilder, scenes
    b = SceneBuilder(be)
    if point:
        b.light_source("point", I=(12, 10, 8), from_=(-1.5, -1.0, 3))
    b.light_source("distant", L=(1.5, 1.5, 2.0), from_=(2, -1, 3), to=(0, 0, 0))
    b.material("matte", Kd=(0.6, 0.6, 0.6))
    scenes._quad(b, (-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0))
    scenes._quad(b, (-0.6, -0.6, 1.0), (0.6, -0.6, 1.0), (0.6, 0.6, 1.0), (-0.6, 0.6, 1.0))
    return b, _cam(be, (0, -5, 4), (0, 0, 0.3), (0, 0, 1), res), res


KD = {"floor": (0.6, 0.5, 0.4), "block": (0.2, 0.5, 0.7)}


def matte_two_lights(be, res=(40, 24)):
    """all matte (sigma = 0) under a point and a distant light: what the per-sample comparison with the oracle's beauty renders"""
    from fountain_amd import SceneBuilder, scenes
    b = SceneBuilder(be)
    b.light_source("point", I=(12, 10, 8), from_=(-1.5, -1.0, 3))
    b.light_source("distant", L=(1.5, 1.5, 2.0), from_=(2, -1, 3), to=(0, 0, 0))
    b.material("matte", Kd=KD["floor"])
    scenes._quad(b, (-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0))
    b.material("matte", Kd=KD["block"])
    scenes._quad(b, (-0.6, -0.6, 1.0), (0.6, -0.6, 1.0), (0.6, 0.6, 1.0), (-0.6, 0.6, 1.0))
    scenes._quad(b, (-0.6, -0.6, 0.0), (0.6, -0.6, 0.0), (0.6, -0.6, 1.0), (-0.6, -0.6, 1.0))
    return b, _cam(be, (0.5, -5, 4), (0, 0, 0.3), (0, 0, 1), res), res
