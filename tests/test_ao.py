"""Ambient occlusion on the GPU (include/fountain_hip_ao.h, fountain_amd/ao.py): closed forms; an independent reconstruction from the
oracle's camera rays, intersections and occlusion tests (tests/_ao_ref.py) -- the three integer fields exactly, bent normals bit for
bit -- on a mixed scene (the four-box any-hit kernel), a triangle-only scene (the eight-box kernel) and a scene behind a null-material
shell; independence of sample splits, tile ranges, crops, the pass plan and the entry; box filters wider than a pixel.  The rays of a
sample do not depend on how many are asked for, so one reference trace per scene and radius serves every ray count."""
import functools

import numpy as np
import pytest

from fountain_amd import Film, FountainError, RandomSampler, scenes, _abi as A
from fountain_amd import ao as AO

import _ao_ref as AR
import _gbuffer_ref as GR

pytestmark = pytest.mark.gpu
F32 = np.float32
INF = float("inf")
bits = GR.bits

SCENES = {"cornell": (AR.cornell, 0.5), "rounded_cube": (AR.rounded_cube, 4.0), "shell": (AR.shell, 1.2)}      # name -> (scene, its finite radius)
SPP, SEED, MAX_RAYS = 3, 2024, 5


@functools.lru_cache(maxsize=None)
def _trace(orc, name, finite, radius=(0.5, 0.5), crop=(0.0, 0.0, 1.0, 1.0), tiles=None):
    make, r = SCENES[name]
    return AR.trace(orc, make, SPP, SEED, MAX_RAYS, r if finite else INF, crop=crop, tiles=tiles, radius=radius)


def _integers(raw):
    return raw[..., [0, 4, 5]]


# ------------------------------------------------------------------ 1. closed forms
def test_open_floor(gpu):
    """nothing occludes a ray that leaves a floor: every ray of every sample is open, and every sample found the floor"""
    b, cam, res = AR.floor(gpu)
    got, raw, st = AO.render_ao(gpu, b, cam, res, RandomSampler(2, 5, indexed=True), rays=3)
    assert st["camera_samples"] == 16 * 16 * 2 == st["rays_closest"]
    assert np.array_equal(raw[..., 4], raw[..., 5]) and raw[..., 5].sum() >= st["camera_samples"]
    assert np.array_equal(raw[..., 0], F32(3.0) * raw[..., 4])
    assert st["rays_any"] == 3 * st["camera_samples"] and st["any_launches"] == 3 and st["any_ms"] > 0
    assert (got["ao"] == 1.0).all() and (got["coverage"] == 1.0).all()
    assert (raw[..., 3] > 0).all() and np.allclose(np.linalg.norm(got["bent"], axis=-1), 1.0, atol=1e-6)
    assert not raw[..., 6:].any()


@pytest.mark.parametrize("radius", [INF, 1.0])
def test_furnace(gpu, orc_det, radius):
    """the camera inside one closed sphere of radius 100.  Unbounded rays all end on it: open == 0 and bent == 0.  With radius 1 a ray
    is occluded only if its chord is shorter than 1, which has probability (1 / 200)^2 per ray: at most one such ray per pixel, on the
    oracle's reference as on the device"""
    rays, spp, seed = 4, 2, 31
    b, cam, res = AR.furnace(gpu)
    _, raw, st = AO.render_ao(gpu, b, cam, res, RandomSampler(spp, seed, indexed=True), rays=rays, radius=radius)
    assert np.array_equal(raw[..., 4], raw[..., 5]) and st["rays_any"] == rays * st["camera_samples"] == rays * 16 * 16 * spp
    if radius == INF:
        assert not raw[..., 0].any() and not raw[..., 1:4].any()
        return
    ref = AR.reconstruct(orc_det, AR.furnace, spp, seed, rays, radius)
    for what, a in (("reference", ref["acc"]), ("device", raw)):
        assert (a[..., 0] >= F32(rays) * a[..., 4] - 1).all(), what
    AR.assert_matches(raw, ref, "furnace, radius 1")


# ------------------------------------------------------------------ 2. parity with the reference
@pytest.mark.parametrize("count_traffic", [0, 1])
@pytest.mark.parametrize("finite", [False, True])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_parity_with_the_reference(gpu, orc_det, name, finite, count_traffic):
    """a 40 x 24 film: four tiles, two of them clipped.  count_traffic = 0: the production any-hit kernels (cornell: four-box, the
    others: eight-box); 1: the reference-order walk"""
    make, r = SCENES[name]
    tr = _trace(orc_det, name, finite)
    b, cam, res = make(gpu)
    scene = b.create_scene()
    for rays in (1, 2, 5):
        what = "%s, %d rays, radius %s, count_traffic %d" % (name, rays, r if finite else "inf", count_traffic)
        ref = AR.sums(tr, rays)
        _, raw, st = AO.render_ao(gpu, None, cam, res, RandomSampler(SPP, SEED, indexed=True), rays=rays, radius=r if finite else INF, scene=scene,
                                  count_traffic=count_traffic)
        print("%s: %d samples, %d surfaces, %d occlusion rays, %d occluded, %d pixels with a foreign sample" % (
            what, ref["n"], ref["hits"], ref["rays_any"], ref["occluded"], int(ref["foreign"].sum())))
        assert (st["camera_samples"], st["rays_closest"], st["rays_any"], st["spill_samples"]) == (ref["n"], ref["rays_closest"], ref["rays_any"], ref["n_spill"]), what
        assert st["any_launches"] == rays, what
        AR.assert_matches(raw, ref, what)
        # the scene exercises what it is here for
        assert 0 < ref["occluded"] < ref["rays_any"] and ref["foreign"].sum() <= 4 * ref["n_spill"], what
        if name == "shell":
            assert ref["rays_closest"] > ref["n"], "no camera ray passed through the shell"
        if name == "rounded_cube":
            assert ref["hits"] < ref["n"], "no camera ray missed"


# ------------------------------------------------------------------ 3. independence
def test_sample_splits_tiles_crop_and_torch(gpu, orc_det):
    import torch
    name, rays = "cornell", 2
    make, r = SCENES[name]
    b, cam, res = make(gpu)
    scene = b.create_scene()
    smp = lambda first=0, count=0: RandomSampler(SPP, SEED, indexed=True, first_sample=first, sample_count=count)
    _, one, st1 = AO.render_ao(gpu, None, cam, res, smp(), rays=rays, scene=scene)
    ref = AR.sums(_trace(orc_det, name, False), rays)
    AR.assert_matches(one, ref, "one call")
    own = ~ref["foreign"]
    # a sample range split over two calls into one buffer
    _, two, sa = AO.render_ao(gpu, None, cam, res, smp(0, 1), rays=rays, scene=scene)
    _, _, sb = AO.render_ao(gpu, None, cam, res, smp(1, SPP - 1), rays=rays, scene=scene, raw=two)
    assert np.array_equal(_integers(two), _integers(one)) and np.array_equal(bits(two[own]), bits(one[own]))
    assert np.allclose(two, one, rtol=2e-6, atol=1e-6)
    assert sa["rays_any"] + sb["rays_any"] == st1["rays_any"] and sa["camera_samples"] + sb["camera_samples"] == st1["camera_samples"]
    # a strided tile range plus its complement
    _, tl, _ = AO.render_ao(gpu, None, cam, res, smp(), rays=rays, scene=scene, tiles=(0, 2, 0))
    AO.render_ao(gpu, None, cam, res, smp(), rays=rays, scene=scene, tiles=(1, 2, 0), raw=tl)
    assert np.array_equal(_integers(tl), _integers(one)) and np.array_equal(bits(tl[own]), bits(one[own]))
    assert np.allclose(tl, one, rtol=2e-6, atol=1e-6)
    # a crop window, against its own reference
    crop = (0.2, 0.1, 0.9, 0.8)
    refc = AR.sums(_trace(orc_det, name, False, crop=crop), rays)
    _, rawc, stc = AO.render_ao(gpu, None, cam, res, smp(), rays=rays, scene=scene, crop=crop)
    assert rawc.shape == refc["acc"].shape and rawc.shape[:2] != one.shape[:2]
    assert (stc["camera_samples"], stc["rays_any"]) == (refc["n"], refc["rays_any"])
    AR.assert_matches(rawc, refc, "crop")
    # the torch entry equals the host entry, the resolve kernel the host resolve
    film = Film(gpu, res)
    t = torch.zeros((film.height, film.width, 8), dtype=torch.float32, device="cuda:0")
    stt = AO.render_ao_torch(scene, cam, film, smp(), t, rays=rays)
    torch.cuda.synchronize()
    assert stt["rays_any"] == st1["rays_any"]
    host = t.cpu().numpy()
    assert np.array_equal(_integers(host), _integers(one)) and np.array_equal(bits(host[own]), bits(one[own])) and np.allclose(host, one, rtol=2e-6, atol=1e-6)
    out = torch.empty((film.height, film.width, 6), dtype=torch.float32, device="cuda:0")
    AO.resolve_torch(gpu, t, rays, out)
    torch.cuda.synchronize()
    res_h = AO.resolve(gpu, host, rays)
    assert np.array_equal(bits(out.cpu().numpy()), bits(np.concatenate([res_h[k] for k in AO.CHANNELS], axis=-1)))
    assert np.array_equal(bits(out.cpu().numpy()), bits(AR.resolve_ref(host, rays).reshape(film.height, film.width, 6)))


def test_several_passes(gpu, monkeypatch):
    """FTN_WF_PATHS_M=1 on a 256^2 film (256 tiles of 256 slots): passes of 16 samples, so 17 spp runs as 16 + 1; the bits are those of
    one pass (device against device)"""
    spp, seed, rays = 17, 8, 2
    b, cam, res = scenes.cornell(gpu, res=256)
    scene = b.create_scene()
    _, one, st1 = AO.render_ao(gpu, None, cam, res, RandomSampler(spp, seed, indexed=True), rays=rays, scene=scene)
    assert st1["camera_samples"] == spp * 256 * 256 and st1["any_launches"] == rays
    monkeypatch.setenv("FTN_WF_PATHS_M", "1")
    _, passes, st = AO.render_ao(gpu, None, cam, res, RandomSampler(spp, seed, indexed=True), rays=rays, scene=scene)
    monkeypatch.delenv("FTN_WF_PATHS_M")
    assert st["any_launches"] == 2 * rays
    assert (st["camera_samples"], st["rays_closest"], st["rays_any"], st["spill_samples"]) == (st1["camera_samples"], st1["rays_closest"], st1["rays_any"], st1["spill_samples"])
    assert np.array_equal(bits(passes), bits(one))
    assert 0 < one[..., 0].sum() < rays * one[..., 4].sum()


# ------------------------------------------------------------------ 4. a box filter wider than a pixel
def test_wide_filter(gpu, orc_det):
    """radius (1.25, 0.5): samples reach the pixels left and right of their own.  The integer fields stay exact; bent is bit-equal where
    no foreign sample landed and within the film's reordering tolerance elsewhere"""
    name, rays, radius = "cornell", 2, (1.25, 0.5)
    make, _ = SCENES[name]
    ref = AR.sums(_trace(orc_det, name, False, radius=radius), rays)
    assert ref["n_spill"] > 0.9 * ref["n"] and ref["foreign"].mean() > 0.9
    b, cam, res = make(gpu)
    _, raw, st = AO.render_ao(gpu, b, cam, res, RandomSampler(SPP, SEED, indexed=True), rays=rays, film=GR.film(gpu, res, (0.0, 0.0, 1.0, 1.0), radius))
    assert (st["camera_samples"], st["rays_any"], st["spill_samples"]) == (ref["n"], ref["rays_any"], ref["n_spill"])
    AR.assert_matches(raw, ref, "radius %r" % (radius,))


# ------------------------------------------------------------------ 5. refusals with a device
def test_refusals(gpu):
    b, cam, res = AR.floor(gpu)
    scene = b.create_scene()
    raw = np.full((16, 16, 8), 3.0, F32)
    for kw, code in ((dict(rays=0), A.FTN_ERR_INVALID_ARGUMENT), (dict(rays=65), A.FTN_ERR_INVALID_ARGUMENT), (dict(radius=0.0), A.FTN_ERR_INVALID_ARGUMENT),
                     (dict(radius=float("nan")), A.FTN_ERR_INVALID_ARGUMENT), (dict(pipeline=A.FTN_PIPELINE_MEGAKERNEL), A.FTN_ERR_UNSUPPORTED)):
        with pytest.raises(FountainError) as e:
            AO.render_ao(gpu, None, cam, res, RandomSampler(2, 5, indexed=True), scene=scene, raw=raw, **kw)
        assert e.value.code == code, kw
    with pytest.raises(FountainError) as e:
        AO.render_ao(gpu, None, cam, res, RandomSampler(2, 5, indexed=False), scene=scene, raw=raw)
    assert e.value.code == A.FTN_ERR_UNSUPPORTED
    assert (raw == 3.0).all()


# ------------------------------------------------------------------ 6. CLI
def test_cli_writes_ao_and_bent(gpu, tmp_path):
    import os
    from fountain_amd import render
    from fountain_amd.api import PbrtScene, read_exr
    scene_file = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "cornell.pbrt")
    out = str(tmp_path / "out.exr")
    assert render.main([scene_file, "-o", out, "--samples", "2", "--ao", "3", "--ao-radius", "0.75"]) == 0
    paths = render.ao_paths(out)
    parsed = PbrtScene(scene_file, gpu)
    want, raw, _ = AO.render_ao(gpu, None, parsed.camera, None, parsed.sampler(2, indexed=True), rays=3, radius=0.75, scene=parsed.create_scene(), film=parsed.film())
    assert np.array_equal(bits(read_exr(paths["ao"], gpu)), bits(np.repeat(want["ao"], 3, axis=-1)))
    assert np.array_equal(bits(read_exr(paths["bent"], gpu)), bits(want["bent"]))
    assert (want["ao"][raw[..., 4] == 0] == 1.0).all() and (want["ao"] >= 0).all() and (want["ao"] <= 1).all() and want["ao"].min() < 1
    assert os.path.exists(out)
