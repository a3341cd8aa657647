"""ID mattes on the GPU (include/fountain_hip_idmatte.h, fountain_amd/idmatte.py): the raw tables against an independent reconstruction
from the oracle's first hits (tests/_idmatte_ref.py), bit for bit, over id kinds, films, crops, tile strides, sample ranges and
filter radii up to 1; tables that overflow; independence of sample splits and of the pass plan; invariants against the beauty and the
G-buffer; resolve and select against their host twins and numpy restatements; refusals; the CLI."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from fountain_amd import FountainError, PathIntegrator, RandomSampler, scenes, _abi as A
from fountain_amd import gbuffer as G
from fountain_amd import idmatte as I

import _gbuffer_ref as GR
import _idmatte_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FULL = (0.0, 0.0, 1.0, 1.0)
MAKE = {"box": R.box, "floor": R.textured_floor, "mesh": R.tessellated}
_hits = {}


def hits(orc, scene, spp, seed, crop=FULL, tiles=None, radius=(0.5, 0.5), first=0, count=0):
    """the oracle's first hits of one configuration, computed once and shared by the tests and id kinds that need them"""
    key = (scene, spp, seed, crop, tiles, radius, first, count)
    if key not in _hits:
        _hits[key] = R.first_hits(orc, MAKE[scene], spp, seed, crop, tiles, radius, first, count)
    return _hits[key]


def render(gpu, scene, kind, spp, seed, crop=FULL, tiles=None, radius=(0.5, 0.5), first=0, count=0, raw=None, sc=None):
    b, cam, res = MAKE[scene](gpu)
    ids, names = I.prim_ids(b, kind)
    smp = RandomSampler(spp, seed, indexed=True, first_sample=first, sample_count=count)
    return I.render_idmatte(gpu, None, cam, res, smp, ids, tiles=tiles, scene=sc or b.create_scene(), film=GR.film(gpu, res, crop, radius), raw=raw)


def assert_equal_tables(got, want, what):
    diff = (got != want).any(-1)
    assert not diff.any(), "%s: %d pixels differ, first %r: got %r, want %r" % (
        what, int(diff.sum()), tuple(np.argwhere(diff)[0]), got[tuple(np.argwhere(diff)[0])], want[tuple(np.argwhere(diff)[0])])


# ------------------------------------------------------------------ 1. reconstruction
@pytest.mark.parametrize("kind", ["material", "shape", "primitive"])
@pytest.mark.parametrize("scene", ["box", "floor"])
def test_reconstruction(gpu, orc_det, scene, kind):
    """a 40 x 27 film (no multiple of 16); the floor scene has a null layer to pass through, a sphere and visible sky"""
    spp, seed = 4, 11
    b, _, _ = MAKE[scene](orc_det)
    ref = R.reconstruct(hits(orc_det, scene, spp, seed), I.prim_ids(b, kind)[0])
    _, raw, st = render(gpu, scene, kind, spp, seed)
    assert st["camera_samples"] == ref["n"] and st["rays_closest"] == ref["rays"] and st["spill_samples"] == ref["n_spill"]
    assert_equal_tables(raw, ref["raw"], "%s %s" % (scene, kind))
    f = I.fields(raw)
    assert (f["miss"] > 0).any() and (f["n_used"] >= 2).any()
    if scene == "floor":
        assert ref["rays"] > ref["n"]                     # some rays passed through the null layer
    if kind == "material":
        assert len(np.unique(f["id"][f["weight"] > 0])) >= (5 if scene == "box" else 3)


@pytest.mark.parametrize("radius", [(0.5, 0.5), (1.0, 1.0), (1.0, 0.5)])
@pytest.mark.parametrize("crop,tiles,first,count", [((0.1, 0.15, 0.95, 0.9), (1, 2, 0), 0, 0), (FULL, (0, 3, 2), 2, 3), (FULL, None, 1, 0)])
def test_reconstruction_crops_strides_ranges_radii(gpu, orc_det, radius, crop, tiles, first, count):
    """with a radius of 1 nearly every sample reaches other pixels: the foreign samples enter in (sample, offset) order after the own"""
    spp, seed, kind = 5, 4242, "primitive"
    b, _, _ = R.box(orc_det)
    ref = R.reconstruct(hits(orc_det, "box", spp, seed, crop, tiles, radius, first, count), I.prim_ids(b, kind)[0])
    _, raw, st = render(gpu, "box", kind, spp, seed, crop, tiles, radius, first, count)
    assert st["camera_samples"] == ref["n"] and st["spill_samples"] == ref["n_spill"]
    if radius[0] > 0.5:
        assert ref["n_spill"] > 0.9 * ref["n"] and ref["foreign"].mean() > 0.3
    assert_equal_tables(raw, ref["raw"], "radius %r crop %r tiles %r" % (radius, crop, tiles))


def test_three_null_layers_pass_through(gpu):
    """three null-material quads over a matte plane (tests/test_gbuffer.py has the same case): four rounds of the pass-through loop, so
    both of its queues are read, refilled and reset in turn; every sample of every pixel ends on the plane, none on a layer"""
    spp = 2
    b, cam, res = GR.null_layers_over_plane(gpu)
    ids, _ = I.prim_ids(b, "shape")
    plane = int(ids[0])
    assert plane not in ids[2:].tolist() and len(ids) == 8          # the plane's two triangles, then the layers': ids of their own
    _, raw, st = I.render_idmatte(gpu, b, cam, res, RandomSampler(spp, 3, indexed=True), ids)
    f = I.fields(raw)
    assert st["camera_samples"] == spp * res[0] * res[1] and st["spill_samples"] == 0
    assert (f["n_used"] == 1).all() and (f["id"][..., 0] == plane).all() and (f["weight"][..., 0] == float(spp)).all()
    assert (f["weight"][..., 1:] == 0.0).all() and (f["overflow"] == 0.0).all()
    assert (f["miss"] == 0.0).all() and (f["total"] == float(spp)).all()
    assert st["rays_closest"] == 4 * st["camera_samples"]          # every camera ray passed through the three quads


def test_device_entry(gpu, orc_det):
    import torch
    spp, seed, radius = 4, 11, (1.0, 1.0)
    b, cam, res = R.textured_floor(gpu)
    ids, _ = I.prim_ids(b, "shape")
    ref = R.reconstruct(hits(orc_det, "floor", spp, seed, radius=radius), ids)
    film = GR.film(gpu, res, FULL, radius)
    out = torch.zeros((film.height, film.width, 20), dtype=torch.float32, device="cuda")
    st = I.render_idmatte_torch(b.create_scene(), cam, film, RandomSampler(spp, seed, indexed=True), ids, out)
    torch.cuda.synchronize()
    raw = out.cpu().numpy().view(np.uint32)
    assert st["camera_samples"] == ref["n"]
    assert_equal_tables(raw, ref["raw"], "device entry")
    # resolve and select on the device against the host twins, on these tables
    res_d = torch.empty_like(out)
    I.resolve_torch(gpu, out, res_d)
    want = I.resolve(gpu, raw)
    assert np.array_equal(res_d.cpu().numpy().view(np.uint32), want)
    mask = torch.empty(out.shape[:2], dtype=torch.float32, device="cuda")
    for kw in (dict(), dict(overflow=True, miss=True)):
        I.select_torch(gpu, res_d, [0, 3, 77], mask, **kw)
        assert np.array_equal(GR.bits(mask.cpu().numpy()), GR.bits(I.select(gpu, want, [0, 3, 77], **kw)))


# ------------------------------------------------------------------ 2. overflow
@pytest.mark.parametrize("radius", [(0.5, 0.5), (1.0, 1.0)])
def test_overflow(gpu, orc_det, radius):
    """a 72 x 72-cell mesh on a 24 x 16 film at 32 spp with primitive ids: a pixel sees more than eight triangles"""
    spp, seed = 32, 5
    b, _, _ = R.tessellated(orc_det)
    ref = R.reconstruct(hits(orc_det, "mesh", spp, seed, radius=radius), I.prim_ids(b, "primitive")[0])
    over = I.fields(ref["raw"])["overflow"] > 0
    assert over.sum() >= 20
    if radius[0] > 0.5:
        assert (over & ref["foreign"]).any()
    _, raw, st = render(gpu, "mesh", "primitive", spp, seed, radius=radius)
    assert st["camera_samples"] == ref["n"]
    assert_equal_tables(raw, ref["raw"], "overflow, radius %r" % (radius,))


# ------------------------------------------------------------------ 3. independence of the plan
@pytest.mark.parametrize("radius", [(0.5, 0.5), (1.0, 1.0)])
def test_sample_split(gpu, radius):
    b, _, _ = R.tessellated(gpu)
    sc = b.create_scene()
    _, one, _ = render(gpu, "mesh", "primitive", 8, 3, radius=radius, sc=sc)
    _, two, _ = render(gpu, "mesh", "primitive", 8, 3, radius=radius, sc=sc, first=0, count=3)
    render(gpu, "mesh", "primitive", 8, 3, radius=radius, sc=sc, first=3, count=5, raw=two)
    if radius[0] <= 0.5:
        assert np.array_equal(one, two)
    else:
        # foreign samples come after the CALL's own samples, so with foreign samples two calls are another order than one: the same
        # samples are in, whatever the order (first-seen order and a full table's choice may differ)
        f1, f2 = I.fields(one), I.fields(two)
        assert np.array_equal(f1["total"], f2["total"]) and np.array_equal(f1["miss"], f2["miss"])
        notfull = (f1["n_used"] < 8) & (f2["n_used"] < 8)
        assert notfull.any()
        r1, r2 = I.resolve(gpu, one), I.resolve(gpu, two)
        assert np.array_equal(r1[notfull], r2[notfull])


def test_several_passes(gpu, monkeypatch):
    """FTN_WF_PATHS_M=1 on a 256^2 film (256 tiles of 256 slots): passes of 16 samples, 20 spp as 16 + 4, against the default plan.
    The mesh spans a quarter of the film's width, some twenty triangles to a pixel."""
    spp, seed = 20, 8
    b, cam, res = R.tessellated(gpu, res=(256, 256), n=200, fov=90.0)
    ids, _ = I.prim_ids(b, "primitive")
    sc = b.create_scene()
    smp = RandomSampler(spp, seed, indexed=True)
    for radius in ((0.5, 0.5), (1.0, 1.0)):
        _, one, st1 = I.render_idmatte(gpu, None, cam, res, smp, ids, scene=sc, film=GR.film(gpu, res, FULL, radius))
        assert (I.fields(one)["overflow"] > 0).sum() >= 20
        monkeypatch.setenv("FTN_WF_PATHS_M", "1")
        _, passes, st = I.render_idmatte(gpu, None, cam, res, smp, ids, scene=sc, film=GR.film(gpu, res, FULL, radius))
        monkeypatch.delenv("FTN_WF_PATHS_M")
        # (a radius of 1 widens the sample bounds by a pixel on every side)
        assert st["camera_samples"] == st1["camera_samples"] == spp * (256 if radius[0] <= 0.5 else 258) ** 2 and st["spill_samples"] == st1["spill_samples"]
        assert np.array_equal(one, passes), radius


# ------------------------------------------------------------------ 4. invariants on rendered buffers
@pytest.mark.parametrize("radius", [(0.5, 0.5), (1.0, 1.0)])
def test_invariants(gpu, radius):
    spp, seed, crop, tiles = 6, 77, (0.05, 0.1, 0.8, 0.97), (0, 2, 0)
    b, cam, res = R.textured_floor(gpu, (64, 48))
    sc = b.create_scene()
    smp = RandomSampler(spp, seed, indexed=True)
    ids, names = I.prim_ids(b, "material")
    _, raw, st = I.render_idmatte(gpu, None, cam, res, smp, ids, tiles=tiles, scene=sc, film=GR.film(gpu, res, crop, radius))
    f = I.fields(raw)
    assert np.array_equal(GR.bits(f["weight"].sum(-1, dtype=F32) + f["overflow"] + f["miss"]), GR.bits(f["total"]))
    film = GR.film(gpu, res, crop, radius)
    from fountain_amd import SamplerIntegrator
    st_b = SamplerIntegrator(cam, PathIntegrator(2, 1.0)).render_parallel(sc, film, smp, tiles=tiles)
    assert np.array_equal(GR.bits(f["total"]), GR.bits(film.pixels[..., 3]))
    _, gb, st_g = G.render_gbuffer(gpu, None, cam, res, smp, tiles=tiles, scene=sc, film=GR.film(gpu, res, crop, radius))
    assert np.array_equal(GR.bits(f["total"]), GR.bits(gb[..., 11])) and np.array_equal(GR.bits(f["total"] - f["miss"]), GR.bits(gb[..., 10]))
    assert st["camera_samples"] == st_b["camera_samples"] == st_g["camera_samples"] and st["spill_samples"] == st_g["spill_samples"]
    assert st["rays_closest"] == st_g["rays_closest"] and st["kernel_ms"] > 0 and 0 < st["trace_ms"] <= st["kernel_ms"]
    used = np.arange(8) < f["n_used"][..., None]
    assert set(np.unique(f["id"][used]).tolist()) <= set(range(sc.desc.n_materials)) and not (f["id"][~used] != 0).any()
    assert (f["total"] > 0).any() and (f["overflow"] == 0).all()


# ------------------------------------------------------------------ 5. resolve and select
def test_resolve_and_select(gpu):
    import torch
    _, rendered, _ = render(gpu, "mesh", "primitive", 16, 9, radius=(1.0, 1.0))
    syn = R.synthetic_tables()
    fs = I.fields(syn)
    tied = [(fs["weight"][i, :n][:, None] == fs["weight"][i, :n][None, :]).sum() > n for i, n in enumerate(np.minimum(fs["n_used"], 8))]
    assert sum(tied) >= 3                                    # the synthetic tables really contain ties in weight
    for raw in (rendered.reshape(-1, 20), syn):
        want = R.resolve_ref(raw)
        host = I.resolve(gpu, raw)
        t = torch.from_numpy(raw.view(F32).copy()).cuda()
        dev = I.resolve_torch(gpu, t, torch.empty_like(t)).cpu().numpy().view(np.uint32)
        assert np.array_equal(host, want) and np.array_equal(dev, want)
        present = np.unique(want[:, 0:16:2])
        for ids in ([], present[::2].tolist(), [0], [0xffffffff, 5, 5, 3], present.tolist()):
            for kw in (dict(), dict(overflow=True), dict(miss=True), dict(overflow=True, miss=True)):
                m_ref = R.select_ref(want, ids, **kw)
                m_host = I.select(gpu, want, ids, **kw)
                rt = torch.from_numpy(want.view(F32).copy()).cuda()
                m_dev = I.select_torch(gpu, rt, ids, torch.empty(rt.shape[0], dtype=torch.float32, device="cuda"), **kw).cpu().numpy()
                assert np.array_equal(GR.bits(m_host), GR.bits(m_ref)) and np.array_equal(GR.bits(m_dev), GR.bits(m_ref)), (ids, kw)
    full = I.select(gpu, R.resolve_ref(rendered), np.unique(I.fields(rendered)["id"]).tolist(), overflow=True, miss=True)
    assert np.abs(full.reshape(rendered.shape[:2])[I.fields(rendered)["total"] > 0] - 1.0).max() <= 1e-6


# ------------------------------------------------------------------ 6. refusals on a GPU
def test_refusals(gpu):
    b, cam, res = R.box(gpu)
    sc = b.create_scene()
    ids, _ = I.prim_ids(b, "material")
    smp = RandomSampler(2, 1, indexed=True)
    raw = np.zeros((res[1], res[0], 20), np.uint32)

    def code(**kw):
        a = dict(be=gpu, builder=None, cam=cam, res=res, sampler=smp, ids=ids, scene=sc, raw=raw)
        a.update(kw)
        with pytest.raises(FountainError) as e:
            I.render_idmatte(**a)
        return e.value.code
    assert code(sampler=RandomSampler(2, 1, indexed=False)) == A.FTN_ERR_UNSUPPORTED
    assert code(pipeline=A.FTN_PIPELINE_MEGAKERNEL) == A.FTN_ERR_UNSUPPORTED
    assert code(ids=ids[:-1]) == A.FTN_ERR_INVALID_ARGUMENT and code(ids=np.concatenate([ids, ids])) == A.FTN_ERR_INVALID_ARGUMENT
    assert code(film=GR.film(gpu, res, FULL, (1.25, 0.5))) == A.FTN_ERR_UNSUPPORTED
    assert code(film=GR.film(gpu, res, FULL, (0.5, 1.0001))) == A.FTN_ERR_UNSUPPORTED
    assert code(sampler=RandomSampler(2, 1, indexed=True, first_sample=1, sample_count=2)) == A.FTN_ERR_INVALID_ARGUMENT
    lib = I._lib(gpu)
    film = GR.film(gpu, res)
    args = [C.byref(cam.desc), C.byref(film.desc), C.byref(smp.desc), None, None]
    p_ids, p_raw = ids.ctypes.data_as(C.c_void_p), raw.ctypes.data_as(C.c_void_p)
    for entry, tail in ((lib.ftn_render_idmatte, (None,)), (lib.ftn_render_idmatte_device, (None, None))):
        assert entry(None, *args, p_ids, ids.size, p_raw, *tail) == A.FTN_ERR_INVALID_ARGUMENT
        assert entry(sc.handle, None, *args[1:], p_ids, ids.size, p_raw, *tail) == A.FTN_ERR_INVALID_ARGUMENT
        assert entry(sc.handle, *args, None, ids.size, p_raw, *tail) == A.FTN_ERR_INVALID_ARGUMENT
        assert entry(sc.handle, *args, p_ids, ids.size, None, *tail) == A.FTN_ERR_INVALID_ARGUMENT
    assert not raw.any()
    assert lib.ftn_idmatte_select_device(p_raw, 1, p_ids, 1, 4, p_raw, None) == A.FTN_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------ 7. the CLI
def test_cli(gpu, tmp_path):
    from fountain_amd import PbrtScene, render as cli
    scene_file = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    out = str(tmp_path / "img.exr")
    assert cli.main([scene_file, "-o", out, "--samples", "4", "--idmatte", "material,shape"]) == 0
    names, planes, attrs = R.read_exr_channels(str(tmp_path / "img_crypto.exr"))
    assert names == sorted(names) and len(names) == 2 * (3 + 16)
    parsed = PbrtScene(scene_file, gpu)
    sc = parsed.create_scene()
    strings = {k: v[1].decode() for k, v in attrs.items() if v[0] == "string"}
    for kind, layer in (("material", "CryptoMaterial"), ("shape", "CryptoObject")):
        ids, id_names = I.prim_ids(parsed, kind)
        resolved, _, _ = I.render_idmatte(gpu, None, parsed.camera, None, parsed.sampler(4, indexed=True), ids, scene=sc, film=parsed.film())
        rk = I.ranks(resolved)
        key = "cryptomatte/%s/" % ("%08x" % I.murmur3_32(layer.encode()))[:7]
        assert strings[key + "name"] == layer and strings[key + "hash"] == "MurmurHash3_32" and strings[key + "conversion"] == "uint32_to_float32"
        manifest = json.loads(strings[key + "manifest"])
        assert manifest == {n: "%08x" % I.name_bits(n) for n in id_names.values()}
        assert len(np.unique(rk["id"][rk["coverage"] > 0])) >= 3
        for r in range(8):
            ch_id, ch_cov = planes["%s%02d.%s" % (layer, r // 2, "RB"[r % 2])], planes["%s%02d.%s" % (layer, r // 2, "GA"[r % 2])]
            assert np.array_equal(GR.bits(ch_cov), GR.bits(rk["coverage"][..., r]))
            want = np.zeros(ch_id.shape, np.uint32)
            for i, n in id_names.items():
                want[(rk["id"][..., r] == i) & (rk["coverage"][..., r] > 0)] = I.name_bits(n)
            assert np.array_equal(GR.bits(ch_id), want) and np.isfinite(ch_id).all()
    # and the mask of two materials through the command line of the module
    mask_file = str(tmp_path / "mask.exr")
    some = sorted(json.loads(strings["cryptomatte/%s/manifest" % ("%08x" % I.murmur3_32(b"CryptoMaterial"))[:7]]))[:2]
    assert I.main([str(tmp_path / "img_crypto.exr"), "--layer", "CryptoMaterial", "--select", *some, "-o", mask_file]) == 0
    from fountain_amd import read_exr
    ids, id_names = I.prim_ids(parsed, "material")
    resolved, _, _ = I.render_idmatte(gpu, None, parsed.camera, None, parsed.sampler(4, indexed=True), ids, scene=sc, film=parsed.film())
    want = I.select(gpu, resolved, [i for i, n in id_names.items() if n in some])
    assert np.array_equal(GR.bits(read_exr(mask_file, gpu)[..., 0]), GR.bits(want)) and want.max() > 0
