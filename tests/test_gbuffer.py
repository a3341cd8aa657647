"""First-hit G-buffers on the GPU (include/fountain_hip_gbuffer.h, fountain_amd/gbuffer.py): an independent reconstruction from the
oracle's camera rays and intersections (tests/_gbuffer_ref.py), bit for bit, with box filters wider than a pixel, crops and tile
strides; the same camera samples as the beauty; spill sums shared with the beauty on one scene handle; several wavefront passes;
null-material pass-through; sample-range splits and the device path; image textures through the camera differentials; the resolve
step; refusals; a config-5-sized scene; the CLI."""
import ctypes as C
import os

import numpy as np
import pytest

from fountain_amd import FountainError, PathIntegrator, RandomSampler, SamplerIntegrator, SceneBuilder, PerspectiveCamera, Film, scenes, _abi as A
from fountain_amd import gbuffer as G

import _gbuffer_ref as GR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO, MEGA, WAVE = A.FTN_PIPELINE_AUTO, A.FTN_PIPELINE_MEGAKERNEL, A.FTN_PIPELINE_WAVEFRONT
F32 = np.float32


bits = GR.bits


# ------------------------------------------------------------------ 1. independent reconstruction
def _hall(be):
    """matte, plastic, metal, mirror and (rough) glass, a partial sphere, a checkerboard floor and a UV-textured wall"""
    b = SceneBuilder(be)
    b.light_source("point", I=(25, 25, 25), from_=(0.3, -0.2, 2.6))
    b.texture("chk", "spectrum", "checkerboard", uscale=6.0, vscale=6.0, tex1=(0.7, 0.7, 0.7), tex2=(0.2, 0.3, 0.45))
    b.texture("uvt", "spectrum", "uv", uscale=2.0, vscale=3.0)
    b.material("matte", Kd="chk")
    scenes._quad(b, (-3, -3, 0), (3, -3, 0), (3, 3, 0), (-3, 3, 0))
    b.material("matte", Kd="uvt")
    scenes._quad(b, (-3, 3, 0), (3, 3, 0), (3, 3, 3), (-3, 3, 3))
    b.material("mirror", Kr=(0.9, 0.85, 0.8))
    scenes._quad(b, (3, -3, 0), (3, 3, 0), (3, 3, 3), (3, -3, 3))
    b.attribute_begin(); b.material("mirror"); b.translate((1.2, 0.5, 0.6)); b.shape("sphere", radius=0.6); b.attribute_end()
    b.attribute_begin(); b.material("plastic", Kd=(0.3, 0.1, 0.1), Ks=(0.4, 0.4, 0.4), roughness=0.05); b.translate((-1.0, 0.2, 0.5)); b.shape("sphere", radius=0.5); b.attribute_end()
    b.attribute_begin(); b.material("metal", eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14), roughness=0.2); b.translate((0.0, 1.6, 0.4)); b.shape("sphere", radius=0.4); b.attribute_end()
    b.attribute_begin(); b.material("glass", Kr=(0.9, 0.95, 1.0), Kt=(1.2, 0.8, -0.1)); b.translate((-0.2, -0.6, 0.35)); b.shape("sphere", radius=0.35); b.attribute_end()
    b.attribute_begin(); b.material("matte", Kd=(0.2, -0.3, 0.8)); b.translate((-1.9, 1.2, 0.7)); b.shape("sphere", radius=0.5, zmin=-0.3, zmax=0.35, phimax=250.0); b.attribute_end()
    b.attribute_begin(); b.material("matte", Kd=(0, 0, 0)); b.area_light_source("diffuse", L=(6, 6, 6)); b.translate((-1.5, -1.0, 2.5)); b.shape("sphere", radius=0.3); b.attribute_end()
    cam = PerspectiveCamera.look_at(be, (0.5, -2.6, 1.6), (0.2, 1.0, 0.7), (0, 0, 1), (72, 56), fov=60.0)
    return b, cam, (72, 56)


@pytest.mark.parametrize("which", ["cornell", "hall"])
def test_independent_reconstruction(gpu, orc_det, which):
    make = {"cornell": lambda be: scenes.cornell(be, res=48), "hall": _hall}[which]
    spp, seed, crop, tiles = 3, 12345, (0.1, 0.15, 0.95, 0.9), (1, 2, 0)
    ref = GR.reconstruct(gpu, orc_det, make, spp, seed, crop, tiles)
    b, cam, res = make(gpu)
    res_g, raw, st = G.render_gbuffer(gpu, b, cam, res, RandomSampler(spp, seed, indexed=True), tiles=tiles, crop=crop)
    assert st["camera_samples"] == ref["n"] and st["spill_samples"] == ref["n_spill"] and st["rays_closest"] == ref["n"]
    GR.assert_matches(raw, ref, which)
    assert np.allclose(raw, ref["acc"], rtol=2e-6, atol=1e-6)
    assert (raw[..., 10] > 0).any()
    assert len({tuple(v) for v in res_g["albedo"][raw[..., 10] > 0].reshape(-1, 3).tolist()}) > 4


@pytest.mark.parametrize("radius", [(1.25, 1.25), (1.5, 0.75), (0.5, 0.5)])
@pytest.mark.parametrize("crop,tiles", [((0.1, 0.15, 0.95, 0.9), (1, 2, 0)), ((0.0, 0.0, 1.0, 1.0), (0, 3, 5))])
def test_reconstruction_with_wide_filters(gpu, orc_det, radius, crop, tiles):
    """footprints clipped to get_film_tile's pixel bounds (p1y with the reference's - radius) and the crop: weights bit-equal
    everywhere, values bit-equal where no sample of another pixel landed and within the reordering bound of a float sum elsewhere"""
    spp, seed = 2, 4242
    ref = GR.reconstruct(gpu, orc_det, _hall, spp, seed, crop, tiles, radius=radius)
    b, cam, res = _hall(gpu)
    _, raw, st = G.render_gbuffer(gpu, None, cam, res, RandomSampler(spp, seed, indexed=True), tiles=tiles, scene=b.create_scene(),
                                  film=GR.film(gpu, res, crop, radius))
    assert st["camera_samples"] == ref["n"] and st["spill_samples"] == ref["n_spill"] and st["rays_closest"] == ref["rays"]
    if radius[0] > 0.5:
        assert ref["n_spill"] > 0.9 * ref["n"] and ref["foreign"].mean() > 0.3
    GR.assert_matches(raw, ref, "radius %r" % (radius,))


# ------------------------------------------------------------------ 2. the beauty's samples
@pytest.mark.parametrize("pipeline", [AUTO, WAVE])
def test_weights_equal_the_beauty(gpu, pipeline):
    spp, crop, tiles = 5, (0.05, 0.1, 0.8, 0.97), (0, 2, 0)
    smp = RandomSampler(spp, 77, indexed=True)
    b, cam, res = scenes.cornell(gpu, res=64)
    _, px, st_b, scene = scenes.render(gpu, b, cam, res, PathIntegrator(3, 1.0), smp, tiles=tiles, crop=crop, backend_kwargs=dict(pipeline=pipeline))
    _, raw, st = G.render_gbuffer(gpu, None, cam, res, smp, tiles=tiles, crop=crop, scene=scene, pipeline=pipeline)
    assert np.array_equal(bits(raw[..., 11]), bits(px[..., 3]))
    assert st["camera_samples"] == st_b["camera_samples"] and st["spill_samples"] == st_b["spill_samples"]
    assert st["kernel_ms"] > 0 and 0 < st["trace_ms"] <= st["kernel_ms"]


@pytest.mark.parametrize("radius", [(1.25, 1.25), (1.5, 0.75)])
@pytest.mark.parametrize("pipeline", [AUTO, WAVE])
def test_weights_equal_the_beauty_with_wide_filters(gpu, pipeline, radius):
    """nearly every sample spills: the whole-number weights still equal the beauty's filter_weight_sum bit for bit"""
    spp, crop, tiles = 5, (0.05, 0.1, 0.8, 0.97), (0, 2, 0)
    smp = RandomSampler(spp, 77, indexed=True)
    b, cam, res = scenes.cornell(gpu, res=64)
    scene = b.create_scene()
    film = GR.film(gpu, res, crop, radius)
    st_b = SamplerIntegrator(cam, PathIntegrator(3, 1.0)).render_parallel(scene, film, smp, tiles=tiles, pipeline=pipeline)
    _, raw, st = G.render_gbuffer(gpu, None, cam, res, smp, tiles=tiles, scene=scene, pipeline=pipeline, film=GR.film(gpu, res, crop, radius))
    assert np.array_equal(bits(raw[..., 11]), bits(film.pixels[..., 3]))
    assert st["camera_samples"] == st_b["camera_samples"] and st["spill_samples"] == st_b["spill_samples"] > 0.9 * st["camera_samples"]


# ------------------------------------------------------------------ 3. null materials
def _null_over_plane(be, kd=(0.4, 0.5, 0.6), h=4.0):
    b = SceneBuilder(be)
    b.light_source("point", I=(5, 5, 5), from_=(0, 0, 3))
    b.material("matte", Kd=kd)
    scenes._quad(b, (-50, -50, 0), (50, -50, 0), (50, 50, 0), (-50, 50, 0))
    b.material("none")
    scenes._quad(b, (-50, -50, 1), (50, -50, 1), (50, 50, 1), (-50, 50, 1))
    cam = PerspectiveCamera.look_at(be, (0, 0, h), (0, 0, 0), (0, 1, 0), (24, 24), fov=50.0)
    return b, cam, (24, 24)


def test_null_material_pass_through(gpu):
    kd, h = (0.4, 0.5, 0.6), 4.0
    b, cam, res = _null_over_plane(gpu, kd, h)
    r, raw, st = G.render_gbuffer(gpu, b, cam, res, RandomSampler(1, 3, indexed=True))
    assert st["spill_samples"] == 0
    hit = raw[..., 10] == 1.0
    assert hit.all() and (raw[..., 11] == 1.0).all()
    assert np.array_equal(bits(raw[..., 0:3]), bits(np.broadcast_to(np.array(kd, F32), raw[..., 0:3].shape)))
    n = raw[..., 3:6].reshape(-1, 3)
    assert np.array_equal(bits(np.abs(n)), bits(np.broadcast_to(np.array([0, 0, 1], F32), n.shape))) and len({tuple(v) for v in n.tolist()}) == 1
    assert np.abs(raw[..., 8]).max() <= 1e-5 * np.abs(raw[..., 6:8]).max()
    assert np.allclose(raw[..., 9], h, rtol=1e-5)
    assert st["rays_closest"] == 2 * st["camera_samples"]          # every camera ray passed through the quad once


def test_three_null_layers_pass_through(gpu):
    """three null-material quads over the plane: four rounds of the pass-through loop, so both of its queues are read, refilled and
    reset in turn (one layer leaves the loop after its first swap)"""
    kd, h, spp = (0.4, 0.5, 0.6), 4.0, 2
    b, cam, res = GR.null_layers_over_plane(gpu, kd, h, (1.0, 2.0, 3.0))
    r, raw, st = G.render_gbuffer(gpu, b, cam, res, RandomSampler(spp, 3, indexed=True))
    assert st["camera_samples"] == spp * res[0] * res[1] and st["spill_samples"] == 0
    assert (raw[..., 10] == float(spp)).all() and (raw[..., 11] == float(spp)).all()          # every sample of every pixel hit
    kd2 = np.array(kd, F32) + np.array(kd, F32)                                                 # the sum of two samples: exact
    assert np.array_equal(bits(raw[..., 0:3]), bits(np.broadcast_to(kd2, raw[..., 0:3].shape)))
    assert np.array_equal(bits(r["albedo"]), bits(np.broadcast_to(np.array(kd, F32), r["albedo"].shape)))
    n = raw[..., 3:6].reshape(-1, 3)
    assert np.array_equal(bits(np.abs(n)), bits(np.broadcast_to(np.array([0, 0, spp], F32), n.shape))) and len({tuple(v) for v in n.tolist()}) == 1
    assert np.abs(raw[..., 8]).max() <= 1e-5 * np.abs(raw[..., 6:8]).max()
    assert np.allclose(raw[..., 9], spp * h, rtol=1e-5)
    assert st["rays_closest"] == 4 * st["camera_samples"]          # every camera ray passed through the three quads


# ------------------------------------------------------------------ 4. splits and the device path
def test_sample_splits_and_device_path(gpu):
    import torch
    n, k, seed, crop = 6, 2, 9, (0.0, 0.0, 1.0, 1.0)
    b, cam, res = _hall(gpu)
    scene = b.create_scene()
    _, one, st1 = G.render_gbuffer(gpu, None, cam, res, RandomSampler(n, seed, indexed=True), scene=scene)
    _, two, _ = G.render_gbuffer(gpu, None, cam, res, RandomSampler(n, seed, indexed=True, first_sample=0, sample_count=k), scene=scene)
    G.render_gbuffer(gpu, None, cam, res, RandomSampler(n, seed, indexed=True, first_sample=k, sample_count=n - k), scene=scene, raw=two)
    if st1["spill_samples"] == 0:
        assert np.array_equal(bits(one), bits(two))
    else:
        assert np.allclose(one, two, rtol=2e-6, atol=1e-6)
    film = Film(gpu, res)
    t = torch.zeros((film.height, film.width, 12), dtype=torch.float32, device="cuda:0")
    G.render_gbuffer_torch(scene, cam, film, RandomSampler(n, seed, indexed=True), t)
    torch.cuda.synchronize()
    assert np.array_equal(bits(t.cpu().numpy()), bits(one))
    out = torch.empty_like(t)
    G.resolve_torch(gpu, t, out)
    torch.cuda.synchronize()
    host = G.resolve(gpu, one)
    want = np.concatenate([host[k2] for k2 in G.CHANNELS], axis=-1)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))


def test_shared_spill_accumulators(gpu, orc_det):
    """the G-buffer's spill sums live in the scene's beauty accumulators, cleared lazily: on one scene handle, G-buffer and beauty calls
    with wide and default filters in turn each equal their own reference, so nothing one call leaves there reaches the next"""
    spp, seed, crop, wide = 2, 31, (0.1, 0.05, 0.9, 0.95), (1.25, 1.25)
    refs = {r: GR.reconstruct(gpu, orc_det, _hall, spp, seed, crop, None, radius=r) for r in (wide, (0.5, 0.5))}
    b, cam, res = _hall(gpu)
    bo, camo, _ = _hall(orc_det)
    scene, scene_o = b.create_scene(), bo.create_scene()
    smp = RandomSampler(spp, seed, indexed=True)
    integ = PathIntegrator(3, 1.0)
    steps = ["gbuffer wide", "beauty default", "gbuffer default", "beauty wide", "gbuffer default", "beauty wide", "gbuffer wide",
             "gbuffer wide"]
    for i, step in enumerate(steps):
        kind, which = step.split()
        radius = wide if which == "wide" else (0.5, 0.5)
        what = "step %d (%s)" % (i, step)
        if kind == "gbuffer":
            _, raw, st = G.render_gbuffer(gpu, None, cam, res, smp, scene=scene, film=GR.film(gpu, res, crop, radius))
            assert st["spill_samples"] == refs[radius]["n_spill"], what
            GR.assert_matches(raw, refs[radius], what)
        else:
            f, fo = GR.film(gpu, res, crop, radius), GR.film(orc_det, res, crop, radius)
            st = SamplerIntegrator(cam, integ).render_parallel(scene, f, smp, pipeline=WAVE)
            SamplerIntegrator(camo, integ).render_parallel(scene_o, fo, smp)
            assert np.array_equal(bits(f.pixels[..., 3]), bits(fo.pixels[..., 3])), what
            if which == "default":
                assert st["spill_samples"] == 0 and np.array_equal(bits(f.pixels), bits(fo.pixels)), what
            else:
                assert np.allclose(f.pixels, fo.pixels, rtol=1e-5, atol=1e-6), what


def test_several_passes(gpu, monkeypatch):
    """FTN_WF_PATHS_M=1 on a 256^2 film (256 tiles of 256 slots): passes of 16 samples, so 37 spp runs as 16 + 16 + 5 (the last with
    a chunk remainder below GB_ACC_CHUNK), and a range starting at sample 5 as 16 + 16 from an offset; every way gives the bits of one
    default pass"""
    spp, seed = 37, 8
    b, cam, res = scenes.cornell(gpu, res=256)
    scene = b.create_scene()
    _, one, st1 = G.render_gbuffer(gpu, None, cam, res, RandomSampler(spp, seed, indexed=True), scene=scene)
    assert st1["camera_samples"] == spp * 256 * 256
    # a sample whose jitter is exactly 0 also lands on the pixel to its left or above: such pixels (weight above spp) get it through
    # the spill sums, which every call adds at its end, so a split call may round them differently
    foreign = one[..., 11] != spp
    assert foreign.sum() <= 4 * st1["spill_samples"]

    def same(got, what, split):
        assert np.array_equal(bits(got[..., 10:]), bits(one[..., 10:])), what
        if split:
            assert np.array_equal(bits(got[~foreign]), bits(one[~foreign])), what
            assert np.allclose(got, one, rtol=2e-6, atol=1e-6), what
        else:
            assert np.array_equal(bits(got), bits(one)), what

    monkeypatch.setenv("FTN_WF_PATHS_M", "1")
    _, passes, st = G.render_gbuffer(gpu, None, cam, res, RandomSampler(spp, seed, indexed=True), scene=scene)
    assert st["camera_samples"] == st1["camera_samples"] and st["rays_closest"] == st1["rays_closest"]
    assert st["spill_samples"] == st1["spill_samples"]
    same(passes, "passes of 16 + 16 + 5", False)
    for k in (5, 16, 21):
        _, two, _ = G.render_gbuffer(gpu, None, cam, res, RandomSampler(spp, seed, indexed=True, first_sample=0, sample_count=k), scene=scene)
        G.render_gbuffer(gpu, None, cam, res, RandomSampler(spp, seed, indexed=True, first_sample=k, sample_count=spp - k), scene=scene, raw=two)
        same(two, "split at %d" % k, True)
    monkeypatch.delenv("FTN_WF_PATHS_M")
    _, two, _ = G.render_gbuffer(gpu, None, cam, res, RandomSampler(spp, seed, indexed=True, first_sample=0, sample_count=5), scene=scene)
    G.render_gbuffer(gpu, None, cam, res, RandomSampler(spp, seed, indexed=True, first_sample=5, sample_count=spp - 5), scene=scene, raw=two)
    same(two, "split at 5, one pass each", True)


# ------------------------------------------------------------------ 5. image textures
def test_constant_image_texture(gpu):
    col = np.array([0.3, 0.55, 0.8], F32)
    b = SceneBuilder(gpu)
    b.light_source("point", I=(5, 5, 5), from_=(0, 0, 3))
    b.texture("img", "spectrum", "imagemap", texels=np.broadcast_to(col, (32, 32, 3)).copy())
    b.material("matte", Kd="img")
    scenes._quad(b, (-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0))
    cam = PerspectiveCamera.look_at(gpu, (0, 0, 1.0), (0, 0, 0), (0, 1, 0), (16, 16), fov=40.0)
    r, raw, st = G.render_gbuffer(gpu, b, cam, (16, 16), RandomSampler(1, 1, indexed=True))
    assert (raw[..., 10] == 1.0).all()
    ulp = np.spacing(col)
    assert (np.abs(r["albedo"] - col) <= 2 * ulp).all(), np.abs(r["albedo"] - col).max(axis=(0, 1)) / ulp


@pytest.mark.parametrize("radius,tiles", [((0.5, 0.5), None), ((1.25, 1.25), (1, 2, 0))])
def test_image_textured_albedo(gpu, orc_det, radius, tiles):
    """a non-constant image map on a grazing floor (MIP levels from the finest to coarse ones) and an image-textured quad under a
    null-material layer (the camera differentials pass through unchanged): the albedo follows the oracle's texture lookup with the
    camera differentials scaled by 1 / sqrt(spp)"""
    spp, seed, crop = 4, 606, (0.0, 0.0, 1.0, 1.0)
    ref = GR.reconstruct(gpu, orc_det, GR.textured_floor, spp, seed, crop, tiles, radius=radius)
    assert ref["rays"] > ref["n"] + 100                                        # samples passed through the null layer
    w = np.log2(np.array(ref["tex_width"]))
    assert w.max() - w.min() > 4, (w.min(), w.max())                          # footprints span several MIP levels
    b, cam, res = GR.textured_floor(gpu)
    _, raw, st = G.render_gbuffer(gpu, None, cam, res, RandomSampler(spp, seed, indexed=True), tiles=tiles, scene=b.create_scene(),
                                  film=GR.film(gpu, res, crop, radius))
    assert st["camera_samples"] == ref["n"] and st["rays_closest"] == ref["rays"] and st["spill_samples"] == ref["n_spill"]
    GR.assert_matches(raw, ref, "image textures, radius %r" % (radius,))


def test_resolve_on_rendered_buffers(gpu):
    """ftn_gbuffer_resolve and ftn_gbuffer_resolve_device against the float32 restatement, bit for bit: sky misses (H = 0), partial
    coverage under a wide filter, pixels of unselected tiles (W = 0)"""
    import torch
    b, cam, res = GR.textured_floor(gpu)
    _, raw, _ = G.render_gbuffer(gpu, None, cam, res, RandomSampler(3, 2, indexed=True), tiles=(0, 2, 0), scene=b.create_scene(),
                                 film=GR.film(gpu, res, (0.0, 0.0, 1.0, 1.0), (1.25, 1.25)))
    h, w = raw[..., 10], raw[..., 11]
    assert (w == 0).any() and ((h == 0) & (w > 0)).any() and ((h > 0) & (h < w)).any() and ((h > 0) & (h == w)).any()
    want = GR.resolve_ref(raw)
    host = G.resolve(gpu, raw)
    assert np.array_equal(bits(np.concatenate([host[k] for k in G.CHANNELS], axis=-1)), bits(want))
    t = torch.from_numpy(raw).cuda()
    out = torch.full_like(t, float("nan"))
    G.resolve_torch(gpu, t, out)
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))


# ------------------------------------------------------------------ 6. refusals
def test_refusals(gpu):
    b, cam, res = scenes.cornell(gpu, res=16)
    scene = b.create_scene()
    with pytest.raises(FountainError) as e:
        G.render_gbuffer(gpu, None, cam, res, RandomSampler(2, 0), scene=scene)
    assert e.value.code == A.FTN_ERR_UNSUPPORTED
    with pytest.raises(FountainError) as e:
        G.render_gbuffer(gpu, None, cam, res, RandomSampler(2, 0, indexed=True), scene=scene, pipeline=MEGA)
    assert e.value.code == A.FTN_ERR_UNSUPPORTED
    film, smp = Film(gpu, res), RandomSampler(2, 0, indexed=True)
    tr, opt, st = A.ftn_tile_range(), A.ftn_render_options(), A.ftn_stats()
    opt.device = -1
    raw = np.zeros((16, 16, 12), F32)
    args = [C.byref(cam.desc), C.byref(film.desc), C.byref(smp.desc), C.byref(tr), C.byref(opt)]
    assert gpu.lib.ftn_render_gbuffer(None, *args, raw.ctypes.data_as(C.c_void_p), C.byref(st)) == A.FTN_ERR_INVALID_ARGUMENT
    assert gpu.lib.ftn_render_gbuffer(scene.handle, *args, None, C.byref(st)) == A.FTN_ERR_INVALID_ARGUMENT
    assert gpu.lib.ftn_render_gbuffer_device(scene.handle, *args, None, None, C.byref(st)) == A.FTN_ERR_INVALID_ARGUMENT
    assert gpu.lib.ftn_render_gbuffer(scene.handle, None, *args[1:], raw.ctypes.data_as(C.c_void_p), C.byref(st)) == A.FTN_ERR_INVALID_ARGUMENT
    assert not raw.any()


# ------------------------------------------------------------------ 7. scale
def test_config5_scene_at_1024(gpu):
    b, cam, res = scenes.instanced_cubes(gpu, res=(1024, 1024))
    r, raw, st = G.render_gbuffer(gpu, b, cam, res, RandomSampler(4, 5, indexed=True))
    assert st["camera_samples"] == 4 * 1024 * 1024
    assert np.isfinite(raw).all() and (raw[..., 10] <= raw[..., 11]).all() and (raw[..., 11] > 0).all()
    hit = r["coverage"][..., 0] > 0
    assert hit.mean() > 0.05
    assert (np.linalg.norm(r["normal"].astype(np.float64), axis=-1) <= 1 + 1e-6).all()
    assert np.isfinite(r["depth"][hit]).all() and (r["depth"][hit] > 0).all() and np.isinf(r["depth"][~hit]).all()


# ------------------------------------------------------------------ 8. CLI
def test_cli_writes_the_four_buffers(gpu, tmp_path):
    from fountain_amd import render
    from fountain_amd.api import PbrtScene, read_exr
    scene_file = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    out = str(tmp_path / "out.exr")
    assert render.main([scene_file, "-o", out, "--samples", "4", "--gbuffer"]) == 0
    paths = render.gbuffer_paths(out)
    parsed = PbrtScene(scene_file, gpu)
    film = parsed.film()
    want, _, _ = G.render_gbuffer(gpu, None, parsed.camera, None, parsed.sampler(4, indexed=True), scene=parsed.create_scene(), film=film)
    for k in ("albedo", "normal", "position"):
        assert np.array_equal(bits(read_exr(paths[k], gpu)), bits(want[k])), k
    d = read_exr(paths["depth"], gpu)
    assert np.array_equal(bits(d), bits(np.repeat(want["depth"], 3, axis=-1)))
    assert os.path.exists(out)
