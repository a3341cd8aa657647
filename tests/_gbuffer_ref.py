"""An independent reconstruction of the first-hit G-buffer (include/fountain_hip_gbuffer.h) from the CPU oracle's camera rays and
intersections, and a float32 numpy restatement of ftn_gbuffer_resolve, shared by test_gbuffer.py and test_gbuffer_cpu.py.

reconstruct() follows film.rs:95-160 in f32 over the samples ftn_render takes: every sample's box-filter footprint is clipped to its
tile's get_film_tile pixel bounds (film.rs:95-113, with the reference's `- radius` in p1y) and then to the crop, and added in tile,
pixel, sample order.  It also returns what a bound on the GPU's reordered spill sums needs: which pixels received a sample of another
pixel, how many terms each pixel summed and the sum of their magnitudes."""
import ctypes as C

import numpy as np

from fountain_amd import Film, _abi as A

F32 = np.float32
U = 2.0 ** -24                     # unit roundoff of binary32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def film(be, res, crop=(0.0, 0.0, 1.0, 1.0), radius=(0.5, 0.5)):
    """Film::new with a BoxFilter of the given radius"""
    f = Film(be, res, crop)
    f.desc.filter_radius[0], f.desc.filter_radius[1] = radius
    return f


def selected_tiles(film, tiles):
    """list_tiles (bounds.rs:85-97) over the film's sample bounds, then the tile range's selection"""
    sb = film.sample_bounds()
    every = [(x, y, min(x + 16, sb[2]), min(y + 16, sb[3])) for y in range(sb[1], sb[3], 16) for x in range(sb[0], sb[2], 16)]
    first, stride, count = tiles if tiles is not None else (0, 1, 0)
    sel = every[first::stride]
    return sel[:count] if count else sel


def tile_pixel_bounds(film, tile):
    """get_film_tile (film.rs:95-113) in f32: the tile's sample bounds widened by the filter radius, intersected with the crop; p1y
    subtracts the radius as the reference does"""
    rx, ry = F32(film.desc.filter_radius[0]), F32(film.desc.filter_radius[1])
    x0, y0, x1, y1 = (F32(v) for v in tile)
    h, one = F32(0.5), F32(1.0)
    p0x, p0y = int(np.ceil(x0 - h - rx)), int(np.ceil(y0 - h - ry))
    p1x, p1y = int(np.ceil(x1 - h + rx + one)), int(np.ceil(y1 - h - ry + one))
    c = film.desc.crop
    return max(p0x, c[0]), max(p0y, c[1]), min(p1x, c[2]), min(p1y, c[3])


def footprint(film, tpb, pfx, pfy):
    """the pixels add_sample (film.rs:133-160) touches for a sample at film position (pfx, pfy), inside the tile bounds tpb"""
    rx, ry = F32(film.desc.filter_radius[0]), F32(film.desc.filter_radius[1])
    pdx, pdy = F32(pfx - F32(0.5)), F32(pfy - F32(0.5))
    x0, y0 = int(np.ceil(pdx - rx)), int(np.ceil(pdy - ry))
    x1, y1 = int(np.floor(pdx + rx)) + 1, int(np.floor(pdy + ry)) + 1
    x0, y0, x1, y1 = max(x0, tpb[0]), max(y0, tpb[1]), min(x1, tpb[2]), min(y1, tpb[3])
    return [(x, y) for y in range(y0, y1) for x in range(x0, x1)]


# ------------------------------------------------------------------ albedo (the table of include/fountain_hip_gbuffer.h, in f32)
def _analytic(b, idx, uv):
    t = b.textures[idx]
    if t.kind == A.FTN_TEX_CONSTANT:
        return np.array(t.value[:], F32)
    s = F32(F32(t.su) * uv[0]) + F32(t.du)
    tt = F32(F32(t.sv) * uv[1]) + F32(t.dv)
    if t.kind == A.FTN_TEX_UV:
        return np.array([s - np.floor(s), tt - np.floor(tt), 0.0], F32)
    assert t.kind == A.FTN_TEX_CHECKERBOARD
    return _analytic(b, t.tex1 if (int(np.floor(s)) + int(np.floor(tt))) % 2 == 0 else t.tex2, uv)


def texture_value(orc, sc, b, idx, uv, diffs):
    """checkerboard / uv / constant restated here (they need no differentials); image maps through the oracle's Texture::evaluate
    with the hit's uv and texture differentials {dudx, dvdx, dudy, dvdy}"""
    if b.textures[idx].kind != A.FTN_TEX_IMAGE:
        return _analytic(b, idx, uv)
    row = (C.c_float * 6)(uv[0], uv[1], *diffs)
    out = (C.c_float * 3)()
    fn = orc.lib.orc_test_texture_eval
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
    assert fn(sc.handle, idx, row, 1, out) == 0
    return np.array(out[:], F32)


def albedo(orc, sc, b, desc, mat, uv, diffs):
    m = desc.materials[mat]
    a, bb = np.array(m.a[:], F32), np.array(m.b[:], F32)
    ta, tb = b.material_textures[mat][0:2]
    if ta >= 0:
        a = texture_value(orc, sc, b, ta, uv, diffs)
    if tb >= 0:
        bb = texture_value(orc, sc, b, tb, uv, diffs)
    pos = lambda v: np.where(v < 0, F32(0), v).astype(F32)
    if m.type in (A.FTN_MAT_MATTE, A.FTN_MAT_MIRROR):
        return pos(a)
    if m.type == A.FTN_MAT_PLASTIC:
        return (a + bb).astype(F32)
    if m.type == A.FTN_MAT_GLASS:
        return (pos(a) + pos(bb)).astype(F32)
    out = (C.c_float * 3)()
    orc.lib.orc_kat_fresnel_conductor(C.c_float(1.0), (C.c_float * 3)(*a), (C.c_float * 3)(*bb), out)
    return np.array(out[:], F32)


def _uses_image(b, mat):
    return any(t >= 0 and b.textures[t].kind == A.FTN_TEX_IMAGE for t in b.material_textures[mat][0:2])


def camera_ray_differential(orc, cam, sample5, spp, hit12=None):
    """orc_kat_camera_ray_differential: (o, d, rx_o, rx_d, ry_o, ry_d) [6, 3] and tex differentials {dudx, dvdx, dudy, dvdy}"""
    out = (C.c_float * 22)()
    h = None if hit12 is None else (C.c_float * 12)(*hit12)
    orc.lib.orc_kat_camera_ray_differential(C.byref(cam.desc), (C.c_float * 5)(*sample5), C.c_uint32(spp), h, out)
    v = np.array(out[:], F32)
    return v[:18].reshape(6, 3), v[18:]


# ------------------------------------------------------------------ the reconstruction
def reconstruct(gpu, orc, make, spp, seed, crop, tiles, radius=(0.5, 0.5), first_sample=0, sample_count=0):
    """The G-buffer sums ftn_render_gbuffer adds for this scene, sampler range, film and tile range, from a zero buffer.  Returns a
    dict: acc [H, W, 12]; foreign [H, W] (the pixel received a sample of another pixel, so the GPU adds it through the spill sums);
    terms [H, W] (hit samples the value channels summed); mag [H, W, 10] (the sum of the magnitudes of those terms); n_spill (samples
    that did not touch exactly one pixel); n (camera samples); rays (closest-hit rays traced, pass-throughs included); tex_width (the
    largest texture differential of every hit on an image-mapped material)."""
    b, cam, res = make(orc)
    sc = b.create_scene()
    f = film(orc, res, crop, radius)
    desc, (_, order) = sc.desc, sc.nodes()
    c2w_inv = A.ftn_transform()
    c2w_inv.m[:] = cam.desc.camera_to_world.inv[:]
    c2w_inv.inv[:] = cam.desc.camera_to_world.m[:]
    u5, p3 = (C.c_float * 5)(), (C.c_float * 3)()
    last = first_sample + (sample_count or spp - first_sample)
    samples, rays = [], []
    for tile in selected_tiles(f, tiles):
        tpb = tile_pixel_bounds(f, tile)
        for py in range(tile[1], tile[3]):
            for px in range(tile[0], tile[2]):
                for s in range(first_sample, last):
                    orc.lib.orc_kat_indexed_f32(C.c_uint64(seed), C.c_int32(px), C.c_int32(py), C.c_uint32(s), u5, C.c_size_t(5))
                    u = np.array(u5[:], F32)
                    s5 = (F32(px) + u[0], F32(py) + u[1], u[2], u[3], u[4])
                    ray, _ = camera_ray_differential(orc, cam, s5, spp)
                    rays.append(list(ray[0]) + list(ray[1]) + [np.inf, 0.0])
                    samples.append((px, py, s5, tpb))
    rays = np.array(rays, F32)
    # first hits that have a material: null-material hits spawn the ray on along its direction (path.rs:77-80)
    full = np.zeros((len(rays), 24), F32)
    prim = np.full(len(rays), -1, np.int64)
    todo, n_rays = np.arange(len(rays)), 0
    spawn = (C.c_float * 8)()
    while todo.size:
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
    c = f.desc.crop
    acc = np.zeros((f.height, f.width, 12), F32)
    foreign = np.zeros((f.height, f.width), bool)
    terms = np.zeros((f.height, f.width), np.int64)
    mag = np.zeros((f.height, f.width, 10), np.float64)
    n_spill, tex_width = 0, []
    for i, (px, py, s5, tpb) in enumerate(samples):
        rec = np.zeros(10, F32)
        hit = prim[i] >= 0
        if hit:
            mat = desc.prims[int(order[prim[i]])].material
            fu = full[i]
            diffs = np.zeros(4, F32)
            if _uses_image(b, mat):
                _, diffs = camera_ray_differential(orc, cam, s5, spp, np.concatenate([fu[0:3], fu[6:9], fu[14:20]]))
                tex_width.append(float(np.abs(diffs).max()))
            gpu.call("transform_point", C.byref(c2w_inv), (C.c_float * 3)(*fu[0:3]), p3)
            rec = np.concatenate([albedo(orc, sc, b, desc, mat, fu[9:11], diffs), fu[20:23], fu[0:3], [p3[2]]]).astype(F32)
        touched = footprint(f, tpb, s5[0], s5[1])
        if len(touched) != 1:
            n_spill += 1
        for (x, y) in touched:
            a = acc[y - c[1], x - c[0]]
            if hit:
                a[:10] += rec * F32(1.0)
                a[10] += F32(1.0)
                terms[y - c[1], x - c[0]] += 1
                mag[y - c[1], x - c[0]] += np.abs(rec.astype(np.float64))
            a[11] += F32(1.0)
            if (x, y) != (px, py):
                foreign[y - c[1], x - c[0]] = True
    return dict(acc=acc, foreign=foreign, terms=terms, mag=mag, n_spill=n_spill, n=len(samples), rays=n_rays, tex_width=tex_width)


def spill_bound(ref):
    """per pixel and value channel, the largest difference between two float32 sums of the same `terms` numbers in different orders:
    each is within gamma(terms - 1) sum|x| of the exact sum, gamma(k) = k u / (1 - k u)"""
    k = np.maximum(ref["terms"] - 1, 0)[..., None].astype(np.float64)
    return 2.0 * k * U / (1.0 - k * U) * ref["mag"]


def assert_matches(raw, ref, what=""):
    """the rules of a reconstruction: weights (10, 11) bit-equal everywhere; value channels bit-equal where no sample of another pixel
    landed, within the reordering bound where one did"""
    want = ref["acc"]
    assert np.array_equal(bits(raw[..., 10:12]), bits(want[..., 10:12])), "%s: weight channels differ at %d pixels" % (
        what, int((bits(raw[..., 10:12]) != bits(want[..., 10:12])).any(-1).sum()))
    diff = (bits(raw[..., :10]) != bits(want[..., :10])).any(-1)
    bad = diff & ~ref["foreign"]
    assert not bad.any(), "%s: %d pixels differ outside spill pixels, first %r" % (what, int(bad.sum()), tuple(np.argwhere(bad)[0]))
    err = np.abs(raw[..., :10].astype(np.float64) - want[..., :10])
    over = err > spill_bound(ref)
    assert not over.any(), "%s: %d spill values beyond the reordering bound, first %r (err %.3g, bound %.3g)" % (
        what, int(over.sum()), tuple(np.argwhere(over)[0]), err[over][0], spill_bound(ref)[over][0])


# ------------------------------------------------------------------ ftn_gbuffer_resolve, restated
def resolve_ref(raw):
    """gbuffer_resolve_pixel in float32: {albedo, normal} / W, {position, depth} / H (zeros and depth inf where H = 0), H / W, W;
    all zeros where W = 0"""
    raw = np.asarray(raw, F32)
    w, h = raw[..., 11:12], raw[..., 10:11]
    out = np.zeros(raw.shape, F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[..., 0:6] = raw[..., 0:6] / w
        out[..., 6:10] = np.where(h == 0, F32(0), raw[..., 6:10] / h)
        out[..., 9:10] = np.where(h == 0, F32(np.inf), out[..., 9:10])
        out[..., 10:11] = h / w
    out[..., 11:12] = w
    out[(w == 0)[..., 0]] = 0
    return out


# ------------------------------------------------------------------ scenes
def textured_floor(be, res=(64, 48), null_layer=True):
    """a grazing floor with a non-constant image map (its far part takes coarse MIP levels), a small image-textured quad under a
    null-material layer, a matte sphere and a sky the camera sees (an infinite light).  Without the null layer (null_layer=False) the
    direct-lighting and Whitted integrators accept it (they refuse a hit without a material)."""
    from fountain_amd import PerspectiveCamera, SceneBuilder, scenes
    rng = np.random.default_rng(17)
    img = rng.random((64, 64, 3)).astype(F32)
    img[::8] *= F32(0.2)
    b = SceneBuilder(be)
    b.light_source("infinite", L=(0.4, 0.5, 0.7))
    b.light_source("point", I=(20, 20, 20), from_=(0.5, -1.0, 3.0))
    b.texture("img", "spectrum", "imagemap", texels=img, uscale=6.0, vscale=6.0)
    b.texture("img2", "spectrum", "imagemap", texels=img[:32, :16].copy(), uscale=2.0, vscale=3.0, wrap="clamp")
    b.material("matte", Kd="img")
    scenes._quad(b, (-20, -4, 0), (20, -4, 0), (20, 40, 0), (-20, 40, 0))
    b.material("matte", Kd="img2")
    scenes._quad(b, (0.3, -1.0, 0.4), (1.3, -1.0, 0.4), (1.3, 0.0, 0.9), (0.3, 0.0, 0.9))
    if null_layer:
        b.material("none")
        scenes._quad(b, (0.2, -1.1, 0.45), (1.4, -1.1, 0.45), (1.4, 0.1, 0.95), (0.2, 0.1, 0.95))
    b.attribute_begin(); b.material("matte", Kd=(0.3, 0.6, 0.3)); b.translate((-0.8, 0.2, 0.35)); b.shape("sphere", radius=0.35); b.attribute_end()
    cam = PerspectiveCamera.look_at(be, (0.0, -3.0, 0.6), (0.0, 6.0, 0.25), (0, 0, 1), res, fov=60.0)
    return b, cam, res


def null_layers_over_plane(be, kd=(0.4, 0.5, 0.6), h=4.0, layers=(1.0, 2.0, 3.0)):
    """a matte plane at z = 0 under one null-material quad per entry of `layers` (its z), seen from straight above at height h on a
    24 x 24 film: every camera ray passes through every layer, one pass-through round each, before it finds the plane"""
    from fountain_amd import PerspectiveCamera, SceneBuilder, scenes
    b = SceneBuilder(be)
    b.light_source("point", I=(5, 5, 5), from_=(0, 0, 3))
    b.material("matte", Kd=kd)
    scenes._quad(b, (-50, -50, 0), (50, -50, 0), (50, 50, 0), (-50, 50, 0))
    b.material("none")
    for z in layers:
        scenes._quad(b, (-50, -50, z), (50, -50, z), (50, 50, z), (-50, 50, z))
    cam = PerspectiveCamera.look_at(be, (0, 0, h), (0, 0, 0), (0, 1, 0), (24, 24), fov=50.0)
    return b, cam, (24, 24)
