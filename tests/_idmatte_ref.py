"""An independent reconstruction of the ID-matte tables (include/fountain_hip_idmatte.h) from the CPU oracle's camera rays and
intersections, numpy restatements of ftn_idmatte_resolve and ftn_idmatte_select, a minimal OpenEXR reader, and the scenes of
test_idmatte.py and test_idmatte_cpu.py.  Nothing here calls the code under test.

first_hits() takes the sample loop of _gbuffer_ref.reconstruct (its helpers are imported, the file is not edited): every camera sample
of ftn_render for the sampler range, film and tile range, its film position, its tile's pixel bounds and the BVH-order primitive of the
first hit that has a material (-1: a miss).  reconstruct() maps order[prim] to the caller's id and applies the table rule: a pixel's own
samples in increasing sample index, then the samples of other pixels ordered by (sample index, source offset (dy, dx) row-major)."""
import ctypes as C
import struct

import numpy as np

from fountain_amd import _abi as A

import _gbuffer_ref as GR

F32 = np.float32
SLOTS, WORDS = 8, 20


# ------------------------------------------------------------------ the oracle's first hits
def first_hits(orc, make, spp, seed, crop, tiles, radius=(0.5, 0.5), first_sample=0, sample_count=0):
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
    prim = np.full(len(rays), -1, np.int64)
    todo, n_rays = np.arange(len(rays)), 0
    spawn = (C.c_float * 8)()
    while todo.size:                       # null-material hits spawn the ray on along its direction (path.rs:77-80)
        n_rays += todo.size
        _, pr, _, _ = sc.intersect(rays[todo], stats=False)
        fu = sc.intersect_full(rays[todo])
        prim[todo] = pr
        again = []
        for k, i in enumerate(todo):
            if pr[k] >= 0 and desc.prims[int(order[pr[k]])].material < 0:
                orc.lib.orc_kat_spawn_ray(*((C.c_float * 3)(*fu[k, a:a + 3]) for a in (0, 3, 6)), (C.c_float * 3)(*rays[i, 3:6]), spawn)
                rays[i] = spawn[:]
                again.append(i)
        todo = np.array(again, np.int64)
    return dict(samples=samples, prim=prim, order=np.asarray(order), film=f, rays=n_rays, n_prims=int(desc.n_prims))


def empty_tables(h, w):
    return np.zeros((h, w, WORDS), np.uint32)


def add(px, hit, x):
    """one sample of weight 1 into the 20 words of a pixel (the rule of the header), in float32"""
    f = px.view(F32)
    one = F32(1.0)
    f[18] += one
    if not hit:
        f[17] += one
        return
    n = int(px[19])
    for k in range(min(n, SLOTS)):
        if px[k] == x:
            f[8 + k] += one
            return
    if n < SLOTS:
        px[n], f[8 + n], px[19] = x, one, n + 1
    else:
        f[16] += one


def reconstruct(hits, ids, start=None):
    """the tables ftn_render_idmatte leaves for these first hits and per-primitive ids (insertion order), continuing `start`.  Returns
    dict: raw [H, W, 20] uint32; foreign [H, W] (the pixel received a sample of another pixel); n, n_spill, rays"""
    f = hits["film"]
    c = f.desc.crop
    raw = empty_tables(f.height, f.width) if start is None else start.copy()
    ids = np.asarray(ids, np.uint32)
    assert ids.shape == (hits["n_prims"],)
    foreign_mask = np.zeros((f.height, f.width), bool)
    later, n_spill = [], 0
    for i, (px, py, s, s5, tpb) in enumerate(hits["samples"]):
        p = int(hits["prim"][i])
        hit = p >= 0
        x = ids[int(hits["order"][p])] if hit else np.uint32(0)
        touched = GR.footprint(f, tpb, s5[0], s5[1])
        if len(touched) != 1:
            n_spill += 1
        for (tx, ty) in touched:
            if (tx, ty) == (px, py):
                add(raw[ty - c[1], tx - c[0]], hit, x)
            else:
                assert abs(px - tx) <= 1 and abs(py - ty) <= 1
                later.append((ty - c[1], tx - c[0], s, py - ty, px - tx, hit, x))
    later.sort(key=lambda e: e[:5])
    for (y, xx, s, dy, dx, hit, x) in later:
        add(raw[y, xx], hit, x)
        foreign_mask[y, xx] = True
    return dict(raw=raw, foreign=foreign_mask, n=len(hits["samples"]), n_spill=n_spill, rays=hits["rays"])


# ------------------------------------------------------------------ ftn_idmatte_resolve / ftn_idmatte_select, restated
def resolve_ref(raw):
    """slots k < min(n_used, 8) ranked by weight descending, ties by id ascending; unused ranks id 0, coverage 0; one float32 divide
    each; total == 0 -> twenty zero words"""
    raw = np.ascontiguousarray(raw, np.uint32).reshape(-1, WORDS)
    out = np.zeros(raw.shape, np.uint32)
    fo, fi = out.view(F32), raw.view(F32)
    for i in range(raw.shape[0]):
        total = fi[i, 18]
        if total == 0:
            continue
        n = min(int(raw[i, 19]), SLOTS)
        slots = sorted(((-float(fi[i, 8 + k]), int(raw[i, k])) for k in range(n)))
        for r, (mw, x) in enumerate(slots):
            out[i, 2 * r] = x
            fo[i, 2 * r + 1] = F32(-mw) / total
        fo[i, 16], fo[i, 17], fo[i, 18], fo[i, 19] = fi[i, 16] / total, fi[i, 17] / total, total, F32(raw[i, 19])
    return out


def select_ref(resolved, ids, overflow=False, miss=False):
    r = np.ascontiguousarray(resolved, np.uint32).reshape(-1, WORDS)
    f = r.view(F32)
    want = set(int(i) for i in ids)
    out = np.zeros(r.shape[0], F32)
    for i in range(r.shape[0]):
        m = F32(0.0)
        for k in range(SLOTS):
            if int(r[i, 2 * k]) in want:
                m = F32(m + f[i, 2 * k + 1])
        if overflow:
            m = F32(m + f[i, 16])
        if miss:
            m = F32(m + f[i, 17])
        out[i] = m
    return out


def synthetic_tables():
    """hand-made tables: ties in weight (ranked by id), total == 0, a full table, n_used == 0, ids 0 and 0xffffffff"""
    rows = []

    def row(ids, ws, overflow, miss, n_used, total=None):
        px = np.zeros(WORDS, np.uint32)
        f = px.view(F32)
        px[:len(ids)] = ids
        f[8:8 + len(ws)] = ws
        f[16], f[17], px[19] = overflow, miss, n_used
        f[18] = (sum(ws[:min(n_used, 8)]) + overflow + miss) if total is None else total
        rows.append(px)
    row([7, 3, 9, 1], [2, 5, 2, 5], 0, 1, 4)                                  # two ties
    row([0xffffffff, 0, 5], [3, 3, 3], 0, 0, 3)                               # a three-way tie with ids 0 and 0xffffffff
    row([4, 8, 15, 16, 23, 42, 1, 2], [1, 2, 3, 4, 5, 6, 7, 8], 3, 2, 8)      # full, with overflow
    row([4, 8, 15, 16, 23, 42, 1, 2], [4, 4, 4, 4, 4, 4, 4, 4], 9, 0, 8)      # full, all tied
    row([], [], 0, 6, 0)                                                      # only misses
    row([5, 6], [1, 1], 0, 0, 2, total=0.0)                                   # total == 0: all zero
    row([], [], 0, 0, 0)                                                      # empty
    row([11, 12, 13], [2, 9, 4], 0, 0, 2)                                     # a stale third slot beyond n_used
    row([0], [5], 0, 2, 1)                                                    # id 0 in use
    return np.array(rows, np.uint32)


# ------------------------------------------------------------------ a minimal OpenEXR reader
def read_exr_channels(path):
    """magic, header attributes, chlist, offset table and uncompressed scanline blocks of FLOAT channels.  Returns
    (channel names in header order, {name: [H, W] float32}, {attribute name: (type, bytes)})"""
    buf = open(path, "rb").read()
    assert buf[:4] == bytes([0x76, 0x2f, 0x31, 0x01]) and buf[4] == 2 and buf[5:8] == b"\0\0\0", "magic / version"
    p, attrs = 8, {}
    while buf[p] != 0:
        e = buf.index(b"\0", p)
        name = buf[p:e].decode()
        p = e + 1
        e = buf.index(b"\0", p)
        typ = buf[p:e].decode()
        size, = struct.unpack_from("<i", buf, e + 1)
        attrs[name] = (typ, buf[e + 5:e + 5 + size])
        p = e + 5 + size
    p += 1
    assert attrs["compression"] == ("compression", b"\0") and attrs["lineOrder"] == ("lineOrder", b"\0")
    assert attrs["channels"][0] == "chlist" and attrs["dataWindow"][0] == "box2i"
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    names, d, q = [], attrs["channels"][1], 0
    while d[q] != 0:
        e = d.index(b"\0", q)
        pixel_type, p_linear, xs, ys = struct.unpack_from("<iB3xii", d, e + 1)
        assert pixel_type == 2 and xs == 1 and ys == 1, "FLOAT, no subsampling"
        names.append(d[q:e].decode())
        q = e + 17
    assert q == len(d) - 1
    planes = {n: np.zeros((h, w), F32) for n in names}
    offsets = struct.unpack_from("<%dQ" % h, buf, p)
    assert offsets[0] == p + 8 * h
    for j, off in enumerate(offsets):
        y, nbytes = struct.unpack_from("<ii", buf, off)
        assert y == y0 + j and nbytes == 4 * w * len(names)
        row = np.frombuffer(buf, F32, w * len(names), off + 8).reshape(len(names), w)
        for k, n in enumerate(names):
            planes[n][j] = row[k]
    assert offsets[-1] + 8 + 4 * w * len(names) == len(buf)
    return names, planes, attrs


# ------------------------------------------------------------------ scenes
def box(be, res=(40, 27)):
    """a Cornell-style box of six materials (five walls and a block), a sphere of a seventh, open to the camera"""
    from fountain_amd import PerspectiveCamera, SceneBuilder, scenes
    b = SceneBuilder(be)
    b.light_source("point", I=(8, 8, 8), from_=(0.0, 0.0, 1.8))
    q = scenes._quad
    b.material("matte", Kd=(0.7, 0.7, 0.7)); q(b, (-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0))          # floor
    b.material("matte", Kd=(0.6, 0.6, 0.7)); q(b, (-1, -1, 2), (1, -1, 2), (1, 1, 2), (-1, 1, 2))          # ceiling
    b.material("matte", Kd=(0.7, 0.1, 0.1)); q(b, (-1, -1, 0), (-1, 1, 0), (-1, 1, 2), (-1, -1, 2))        # left
    b.material("matte", Kd=(0.1, 0.7, 0.1)); q(b, (1, -1, 0), (1, 1, 0), (1, 1, 2), (1, -1, 2))            # right
    b.material("plastic", Kd=(0.3, 0.3, 0.6), Ks=(0.3, 0.3, 0.3), roughness=0.1); q(b, (-1, 1, 0), (1, 1, 0), (1, 1, 2), (-1, 1, 2))   # back
    b.material("mirror", Kr=(0.9, 0.9, 0.9))
    q(b, (-0.6, -0.2, 0.6), (0.0, -0.4, 0.6), (0.2, 0.2, 0.6), (-0.4, 0.4, 0.6))                           # a block's top
    q(b, (-0.6, -0.2, 0.0), (0.0, -0.4, 0.0), (0.0, -0.4, 0.6), (-0.6, -0.2, 0.6))                         # and its front
    b.attribute_begin(); b.material("metal", eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14), roughness=0.2); b.translate((0.45, -0.1, 0.3)); b.shape("sphere", radius=0.3); b.attribute_end()
    cam = PerspectiveCamera.look_at(be, (0.0, -3.4, 1.0), (0.0, 0.0, 1.0), (0, 0, 1), res, fov=40.0)
    return b, cam, res


def textured_floor(be, res=(40, 27)):
    return GR.textured_floor(be, res)


def tessellated(be, res=(24, 16), n=72, fov=32.0):
    """an n x n grid of cells, two triangles each, as one mesh, seen square on from far enough that a pixel covers a dozen triangles;
    the film is wider than the mesh, so the outer columns see the sky"""
    from fountain_amd import PerspectiveCamera, SceneBuilder
    b = SceneBuilder(be)
    b.light_source("infinite", L=(0.5, 0.5, 0.5))
    b.material("matte", Kd=(0.5, 0.5, 0.5))
    g = np.linspace(-1.0, 1.0, n + 1, dtype=F32)
    P = [(float(x), float(y), 0.0) for y in g for x in g]
    idx = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            idx += [a, a + 1, a + n + 2, a, a + n + 2, a + n + 1]
    b.shape("trianglemesh", P=P, indices=idx)
    cam = PerspectiveCamera.look_at(be, (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (0, 1, 0), res, fov=fov)
    return b, cam, res
