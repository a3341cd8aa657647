"""An independent reconstruction of the ambient-occlusion pass (include/fountain_hip_ao.h) from the CPU oracle's camera rays,
intersections and occlusion tests, a float32 numpy restatement of ftn_ao_resolve, and the scenes of test_ao.py and test_ao_cpu.py.
Nothing here calls the code under test.

first_surfaces() takes the sample loop of _gbuffer_ref.reconstruct and _idmatte_ref.first_hits (their helpers are imported, the files
are not edited) and keeps every sample's interaction record.  ao_ray_ref() restates the header's ray: faceforward and coordinate_system
in numpy float32 (division and square root are correctly rounded on both sides), the oracle's cosine_sample_hemisphere and spawn_ray.
trace() sends those rays through the oracle's intersect_test and sums() applies the film rule: a pixel's own samples in increasing
sample index into what the buffer holds, the samples of other pixels summed apart and added after."""
import ctypes as C

import numpy as np

import _gbuffer_ref as GR

F32 = np.float32
INF = float("inf")


# ------------------------------------------------------------------ the header's ray, restated
def _dot(a, b):
    return F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))


def _normalize(v):
    inv = F32(F32(1.0) / np.sqrt(_dot(v, v), dtype=F32))
    return np.array([v[0] * inv, v[1] * inv, v[2] * inv], F32)


def faceforward(n, wo):
    return -n if _dot(n, wo) < 0 else n


def coordinate_system(v1):
    z = F32(0.0)
    if abs(v1[0]) > abs(v1[1]):
        v2 = _normalize(np.array([-v1[2], z, v1[0]], F32))
    else:
        v2 = _normalize(np.array([z, v1[2], -v1[1]], F32))
    v3 = np.array([F32(v1[1] * v2[2]) - F32(v1[2] * v2[1]), F32(v1[2] * v2[0]) - F32(v1[0] * v2[2]), F32(v1[0] * v2[1]) - F32(v1[1] * v2[0])], F32)
    return v2, v3


def ao_direction(orc, n, wo, u):
    """(nf, l, d): d = (s l.x + t l.y) + nf l.z per component"""
    n, wo = np.asarray(n, F32), np.asarray(wo, F32)
    nf = faceforward(n, wo)
    s, t = coordinate_system(nf)
    l3 = (C.c_float * 3)()
    orc.lib.orc_kat_cosine_hemisphere(C.c_float(u[0]), C.c_float(u[1]), l3)
    l = np.array(l3[:], F32)
    d = np.array([F32(F32(F32(s[k] * l[0]) + F32(t[k] * l[1])) + F32(nf[k] * l[2])) for k in range(3)], F32)
    return nf, l, d


def ao_ray_ref(orc, fu, u, radius=INF):
    """the occlusion ray {o, d, radius, 0} of the interaction record fu (ftn_intersect_full's 24 floats) for the draws u"""
    fu = np.asarray(fu, F32)
    _, _, d = ao_direction(orc, fu[6:9], fu[11:14], u)
    out = (C.c_float * 8)()
    orc.lib.orc_kat_spawn_ray(*((C.c_float * 3)(*fu[a:a + 3]) for a in (0, 3, 6)), (C.c_float * 3)(*d), out)
    r = np.array(out[:], F32)
    assert np.array_equal(GR.bits(r[3:6]), GR.bits(d))
    r[6], r[7] = radius, 0.0
    return r


# ------------------------------------------------------------------ the oracle's first surfaces
def first_surfaces(orc, make, spp, seed, crop, tiles, radius=(0.5, 0.5), first_sample=0, sample_count=0):
    b, cam, res = make(orc)
    sc = b.create_scene()
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
    full = np.zeros((len(rays), 24), F32)
    prim = np.full(len(rays), -1, np.int64)
    todo, n_rays = np.arange(len(rays)), 0
    spawn = (C.c_float * 8)()
    while todo.size:                       # null-material hits spawn the ray on along its direction (path.rs:77-80)
        n_rays += todo.size
        _, pr, _, _ = sc.intersect(rays[todo], stats=False)
        fu = sc.intersect_full(rays[todo])
        full[todo], prim[todo] = fu, pr
        again = []
        for k, i in enumerate(todo):
            if pr[k] >= 0 and desc.prims[int(order[pr[k]])].material < 0:
                orc.lib.orc_kat_spawn_ray(*((C.c_float * 3)(*fu[k, a:a + 3]) for a in (0, 3, 6)), (C.c_float * 3)(*rays[i, 3:6]), spawn)
                rays[i] = spawn[:]
                again.append(i)
        todo = np.array(again, np.int64)
    return dict(samples=samples, prim=prim, full=full, film=f, rays=n_rays, scene=sc, keep=(b, cam))


def trace(orc, make, spp, seed, rays, ao_radius=INF, crop=(0.0, 0.0, 1.0, 1.0), tiles=None, radius=(0.5, 0.5), first_sample=0, sample_count=0):
    """the first surfaces, and for each the `rays` occlusion rays of the header with the oracle's intersect_test answer.  Ray k of a
    sample does not depend on `rays`, so one trace serves every smaller ray count (sums)."""
    fs = first_surfaces(orc, make, spp, seed, crop, tiles, radius, first_sample, sample_count)
    hit_idx = [i for i in range(len(fs["samples"])) if fs["prim"][i] >= 0]
    draws = (C.c_float * (5 + 2 * rays))()
    ao = np.zeros((len(hit_idx), rays, 8), F32)
    for j, i in enumerate(hit_idx):
        px, py, s, _, _ = fs["samples"][i]
        orc.lib.orc_kat_indexed_f32(C.c_uint64(seed), C.c_int32(px), C.c_int32(py), C.c_uint32(s), draws, C.c_size_t(5 + 2 * rays))
        for k in range(rays):
            ao[j, k] = ao_ray_ref(orc, fs["full"][i], (draws[5 + 2 * k], draws[6 + 2 * k]), ao_radius)
    occ = fs["scene"].intersect_test(ao.reshape(-1, 8), stats=False)[0].reshape(len(hit_idx), rays) if len(hit_idx) else np.zeros((0, rays), bool)
    return dict(fs=fs, hit_idx=hit_idx, ao=ao, occ=occ, rays=rays)


def sums(tr, rays=None, start=None):
    """The sums ftn_render_ao adds for a trace with its first `rays` rays per surface, into `start` (zeros when None).  Returns a dict:
    acc [H, W, 8]; foreign [H, W] (the pixel received a sample of another pixel, so the device adds it through the spill sums);
    n (camera samples), n_spill, rays_closest, rays_any, hits, occluded."""
    fs, hit_idx, ao, occ = tr["fs"], tr["hit_idx"], tr["ao"], tr["occ"]
    rays = rays or tr["rays"]
    assert rays <= tr["rays"]
    f = fs["film"]
    c = f.desc.crop
    acc = np.zeros((f.height, f.width, 8), F32) if start is None else np.array(start, F32)
    spill = np.zeros((f.height, f.width, 8), F32)
    foreign = np.zeros((f.height, f.width), bool)
    per_sample, n_spill = [None] * len(fs["samples"]), 0
    for j, i in enumerate(hit_idx):
        count, bent = F32(0.0), np.zeros(3, F32)
        for k in range(rays):
            if not occ[j, k]:
                count = F32(count + F32(1.0))
                bent = (bent + ao[j, k, 3:6]).astype(F32)
        per_sample[i] = (count, bent)
    for i, (px, py, s, s5, tpb) in enumerate(fs["samples"]):
        touched = GR.footprint(f, tpb, s5[0], s5[1])
        if len(touched) != 1:
            n_spill += 1
        for (x, y) in touched:
            own = (x, y) == (px, py)
            a = (acc if own else spill)[y - c[1], x - c[0]]
            if per_sample[i] is not None:
                a[0] += per_sample[i][0] * F32(1.0)
                a[1:4] += per_sample[i][1] * F32(1.0)
                a[4] += F32(1.0)
            a[5] += F32(1.0)
            if not own:
                foreign[y - c[1], x - c[0]] = True
    acc[..., :6] += spill[..., :6]
    return dict(acc=acc, foreign=foreign, n=len(fs["samples"]), n_spill=n_spill, rays_closest=fs["rays"], rays_any=len(hit_idx) * rays, hits=len(hit_idx),
                occluded=int(occ[:, :rays].sum()))


def reconstruct(orc, make, spp, seed, rays, ao_radius=INF, start=None, **kw):
    return sums(trace(orc, make, spp, seed, rays, ao_radius, **kw), rays, start)


def assert_matches(raw, ref, what="", rtol=2e-6, atol=1e-6):
    """open, hit_weight and weight equal as integers on every pixel; bent bit-equal where no sample of another pixel landed and within
    the tolerance of the film's reordered spill sums (tests/test_gbuffer.py's) where one did; the padding untouched"""
    want = ref["acc"]
    for k, name in ((0, "open"), (4, "hit_weight"), (5, "weight")):
        assert np.array_equal(raw[..., k], np.round(raw[..., k])) and np.array_equal(raw[..., k].astype(np.int64), want[..., k].astype(np.int64)), \
            "%s: %s differs at %d pixels" % (what, name, int((raw[..., k] != want[..., k]).sum()))
    diff = (GR.bits(raw[..., 1:4]) != GR.bits(want[..., 1:4])).any(-1)
    bad = diff & ~ref["foreign"]
    assert not bad.any(), "%s: bent differs at %d pixels outside spill pixels, first %r" % (what, int(bad.sum()), tuple(np.argwhere(bad)[0]))
    assert np.allclose(raw[..., 1:4], want[..., 1:4], rtol=rtol, atol=atol), "%s: bent beyond the spill tolerance" % what
    assert np.array_equal(GR.bits(raw[..., 6:8]), GR.bits(want[..., 6:8])), "%s: padding written" % what


# ------------------------------------------------------------------ ftn_ao_resolve, restated
def resolve_ref(raw, rays):
    """ao_resolve_pixel in float32: open / (rays * H), bent * (1 / sqrt((x x + y y) + z z)) or 0, H / W, W; H = 0: ao 1, bent 0; W = 0: zeros"""
    raw = np.asarray(raw, F32).reshape(-1, 8)
    out = np.zeros((len(raw), 6), F32)
    for i, r in enumerate(raw):
        h, w = r[4], r[5]
        if w == 0:
            continue
        if h == 0:
            out[i, 0] = 1.0
        else:
            with np.errstate(all="ignore"):
                out[i, 0] = r[0] / F32(F32(rays) * h)
                l = np.sqrt(_dot(r[1:4], r[1:4]), dtype=F32)
                if l != 0:
                    inv = F32(F32(1.0) / l)
                    out[i, 1:4] = r[1:4] * inv
        with np.errstate(all="ignore"):
            out[i, 4] = h / w
        out[i, 5] = w
    return out


def synthetic_sums():
    """hand-made sums: weight == 0 (with stale values), hit_weight == 0, a zero-length bent, an underflowing length, ordinary pixels"""
    rows = [
        [7, 1, 2, 3, 2, 0, 9, 9],                        # weight == 0: six zeros
        [0, 0, 0, 0, 0, 5, 0, 0],                        # only misses: ao 1, bent 0, coverage 0
        [0, 0, 0, 0, 3, 4, 0, 0],                        # every ray occluded: bent of length 0
        [6, 0.5, -0.25, 2.0, 2, 2, 0, 0],
        [5, -1.0, 1.0, 1.0, 3, 7, 0, 0],
        [1, 1e-30, 0, 0, 1, 1, 0, 0],                    # x * x underflows to 0: length 0
        [64 * 9, 3.0, 4.0, 12.0, 9, 9, 0, 0],            # ao exactly 1
        [1, 0.3, 0.3, 0.3, 3, 3, 0, 0],
    ]
    rng = np.random.default_rng(5)
    more = np.concatenate([rng.integers(0, 40, (64, 1)), rng.normal(size=(64, 3)) * 3, rng.integers(1, 10, (64, 1)), rng.integers(10, 20, (64, 1)),
                           np.zeros((64, 2))], axis=1)
    return np.concatenate([np.array(rows, np.float64), more]).astype(F32)


# ------------------------------------------------------------------ scenes
def floor(be, res=(16, 16)):
    """one large two-triangle floor seen from above: nothing occludes a ray that leaves it"""
    from fountain_amd import PerspectiveCamera, SceneBuilder, scenes
    b = SceneBuilder(be)
    b.light_source("point", I=(5, 5, 5), from_=(0, 0, 3))
    b.material("matte", Kd=(0.5, 0.5, 0.5))
    scenes._quad(b, (-50, -50, 0), (50, -50, 0), (50, 50, 0), (-50, 50, 0))
    cam = PerspectiveCamera.look_at(be, (0, 0, 4), (0, 0, 0), (0, 1, 0), res, fov=50.0)
    return b, cam, res


def cornell(be, res=(40, 24)):
    """triangles and spheres: the four-box any-hit kernel"""
    from fountain_amd import PerspectiveCamera, scenes
    b, _, _ = scenes.cornell(be, res=res[0])
    cam = PerspectiveCamera.look_at(be, (0, -3.4, 0), (0, 0, 0), (0, 0, 1), res, fov=40.0)
    return b, cam, res


def rounded_cube(be, res=(40, 24)):
    """the rounded cube on its ground under the environment light, triangles only: the eight-box any-hit kernel"""
    from fountain_amd import PerspectiveCamera, scenes
    b, _, _ = scenes.rounded_cube_env(be, res=res[0], env_n=16)
    cam = PerspectiveCamera.look_at(be, (28, -28, 14), (0, 0, -2), (0, 0, 1), res, fov=40.0)
    return b, cam, res


def shell(be, res=(40, 24)):
    """a matte block on a floor inside a null-material box: every camera ray passes through the shell first, and the occlusion rays that
    leave the block or the floor are stopped by the shell from inside (every primitive occludes)"""
    from fountain_amd import PerspectiveCamera, SceneBuilder, scenes
    b = SceneBuilder(be)
    b.light_source("infinite", L=(0.5, 0.5, 0.5))
    q = scenes._quad
    b.material("matte", Kd=(0.6, 0.6, 0.6))
    q(b, (-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0))                                   # floor, wider than the shell
    b.material("matte", Kd=(0.7, 0.3, 0.2))
    q(b, (-0.5, -0.5, 0.8), (0.5, -0.5, 0.8), (0.5, 0.5, 0.8), (-0.5, 0.5, 0.8))           # a block's top
    q(b, (-0.5, -0.5, 0.0), (0.5, -0.5, 0.0), (0.5, -0.5, 0.8), (-0.5, -0.5, 0.8))         # and its front
    b.material("none")
    q(b, (-1.5, -1.5, 0.0), (1.5, -1.5, 0.0), (1.5, -1.5, 2.0), (-1.5, -1.5, 2.0))         # the shell: front
    q(b, (-1.5, -1.5, 2.0), (1.5, -1.5, 2.0), (1.5, 1.5, 2.0), (-1.5, 1.5, 2.0))           # top
    q(b, (-1.5, -1.5, 0.0), (-1.5, 1.5, 0.0), (-1.5, 1.5, 2.0), (-1.5, -1.5, 2.0))         # left
    cam = PerspectiveCamera.look_at(be, (0.3, -5.0, 2.2), (0.0, 0.0, 0.5), (0, 0, 1), res, fov=40.0)
    return b, cam, res


def furnace(be, res=(16, 16)):
    from fountain_amd import scenes
    b, cam, r = scenes.furnace(be, res=res[0])
    return b, cam, r
