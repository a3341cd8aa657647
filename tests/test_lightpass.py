"""The light-group pass on the GPU (include/fountain_hip_lightpass.h, fountain_amd/lightpass.py): a sample-by-sample replay from the
oracle's camera rays, intersections, light samples and occlusion tests (tests/_lightpass_ref.py) -- the weights and, in sample order, the
float sums bit for bit -- on scenes with every kind of light and both any-hit kernels; exact properties; Kd / pi * lit against the
oracle's beauty of the same sample; independence of crops, sample splits, tile ranges, the pass plan, the traversal and the entry; the two
image-space stages against their host twins; refusals; the command line."""
import functools
import os

import numpy as np
import pytest

from fountain_amd import Film, FountainError, PathIntegrator, RandomSampler, _abi as A
from fountain_amd import lightpass as LP

import _ao_ref as AR
import _gbuffer_ref as GR
import _lightpass_ref as LR
import _moments_ref as MR

pytestmark = pytest.mark.gpu
F32 = np.float32
bits = GR.bits
U = 2.0 ** -24

SCENES = {"floor_blocker": LR.floor_blocker, "cornell": AR.cornell, "rounded_cube": AR.rounded_cube, "null_quad": LR.null_quad, "every_kind": LR.every_kind}
SPP, SEED = 4, 2024


def _smp(first=0, count=0, spp=SPP, seed=SEED):
    return RandomSampler(spp, seed, indexed=True, first_sample=first, sample_count=count)


@functools.lru_cache(maxsize=None)
def _replay(orc, ftn, name, lights=None, crop=(0.0, 0.0, 1.0, 1.0), tiles=None):
    return LR.replay(orc, ftn, SCENES[name], SPP, SEED, lights, crop=crop, tiles=tiles)


@functools.lru_cache(maxsize=None)
def _scene(gpu, name):
    b, cam, res = SCENES[name](gpu)
    return b.create_scene(), cam, res


# ------------------------------------------------------------------ 1. the replay
@pytest.mark.parametrize("name,lights", [("floor_blocker", None), ("cornell", None), ("rounded_cube", None), ("null_quad", None), ("every_kind", None),
                                         ("every_kind", (1, 3))])
def test_replay(gpu, orc_det, name, lights):
    """40 x 24 films at 4 spp: four tiles, two of them clipped.  cornell has spheres (the four-box any-hit kernel), the others are
    triangles only (the eight-box one)"""
    ref = _replay(orc_det, gpu, name, lights)
    scene, cam, res = _scene(gpu, name)
    what = "%s, lights %r" % (name, lights)
    got, raw, st = LP.render_lightpass(gpu, None, cam, res, _smp(), lights=lights, scene=scene)
    print("%s: %d samples, %d surfaces, %d shadow rays, %d occluded, %d pixels with a foreign sample" % (
        what, ref["n"], ref["hits"], ref["rays_any"], ref["occluded"], int((ref["foreign"] > 0).sum())))
    assert (st["camera_samples"], st["rays_closest"], st["rays_any"], st["spill_samples"]) == (ref["n"], ref["rays_closest"], ref["rays_any"], ref["n_spill"]), what
    assert st["any_launches"] == 1 and st["any_ms"] > 0, what
    LR.assert_matches(raw, ref, what)
    # the scene exercises what it is here for
    assert 0 < ref["occluded"] < ref["rays_any"] and (ref["foreign"] > 1).sum() <= ref["n_spill"], what
    assert ref["acc"][..., 0:3].sum() > 0 and (ref["acc"][..., 0:3] <= ref["acc"][..., 3:6]).all()
    if name == "null_quad":
        assert ref["rays_closest"] > ref["n"], "no camera ray passed through the quad"
    if name == "rounded_cube":
        assert ref["hits"] < ref["n"], "no camera ray missed"
    if name in ("rounded_cube", "every_kind"):
        assert ref["rays_any"] < ref["hits"], "no light sample was refused"


def test_replay_with_a_wide_filter(gpu, orc_det):
    """cornell under a box filter of radius (0.75, 0.5): half the samples reach a neighbour in x, so most pixels' sums come through the
    spill sums and their merge.  A pixel that one foreign sample reached is held to bits, and among those pixels are shadowed ones: a
    lit that the spill path added for an occluded sample (or added as + 0.0 onto a -0.0) would show there"""
    radius = (0.75, 0.5)
    ref = LR.replay(orc_det, gpu, AR.cornell, SPP, SEED, None, radius=radius)
    scene, cam, res = _scene(gpu, "cornell")
    _, raw, st = LP.render_lightpass(gpu, None, cam, res, _smp(), scene=scene, film=GR.film(gpu, res, (0.0, 0.0, 1.0, 1.0), radius))
    one, many = ref["foreign"] == 1, ref["foreign"] > 1
    shadowed = (ref["acc"][..., 0:3] < ref["acc"][..., 3:6]).any(-1)
    print("radius %r: %d samples, %d spilled, %d shadow rays, %d occluded; pixels with 0 / 1 / more foreign samples %d / %d / %d, shadowed among the last two %d / %d" % (
        radius, ref["n"], ref["n_spill"], ref["rays_any"], ref["occluded"], int((ref["foreign"] == 0).sum()), int(one.sum()), int(many.sum()),
        int((one & shadowed).sum()), int((many & shadowed).sum())))
    assert (st["camera_samples"], st["rays_closest"], st["rays_any"], st["spill_samples"]) == (ref["n"], ref["rays_closest"], ref["rays_any"], ref["n_spill"])
    assert st["any_launches"] == 1 and st["any_ms"] > 0
    LR.assert_matches(raw, ref, "cornell, radius %r" % (radius,))
    # the reference reaches what the test is here for
    assert ref["n_spill"] > 0.4 * ref["n"] and one.sum() >= 100 and many.sum() >= 100
    assert (one & shadowed).sum() >= 5 and (many & shadowed).sum() >= 5


# ------------------------------------------------------------------ 2. exact properties
def test_open_and_covered(gpu):
    """nothing between surface and lights: lit == unshadowed bit for bit.  A plate that covers the light: lit == 0 while unshadowed > 0"""
    b, cam, res = LR.open_floor(gpu)
    _, raw, st = LP.render_lightpass(gpu, b, cam, res, _smp())
    assert np.array_equal(bits(raw[..., 0:3]), bits(raw[..., 3:6])) and (raw[..., 3:6] > 0).all()
    assert np.array_equal(raw[..., 6], raw[..., 7]) and st["rays_any"] == st["camera_samples"] == 24 * 16 * SPP
    b, cam, res = LR.covered_floor(gpu)
    got, raw, st = LP.render_lightpass(gpu, b, cam, res, _smp())
    assert not raw[..., 0:3].any() and (raw[..., 3:6] > 0).all() and st["rays_any"] == st["camera_samples"]
    assert not got["visibility"].any() and (got["coverage"] == 1).all()


def test_light_lists_and_weights(gpu):
    """lights = NULL equals the explicit full list; [1] of {point, distant} equals all lights of the scene with the distant light alone;
    the weights are the G-buffer's; a scene without lights adds the weights and traces nothing"""
    from fountain_amd.gbuffer import render_gbuffer
    scene, cam, res = _scene(gpu, "every_kind")
    _, full, st = LP.render_lightpass(gpu, None, cam, res, _smp(), scene=scene)
    _, listed, st2 = LP.render_lightpass(gpu, None, cam, res, _smp(), lights=[0, 1, 2, 3, 4], scene=scene)
    assert np.array_equal(bits(full), bits(listed)) and st["rays_any"] == st2["rays_any"] > 0
    _, gb, _ = render_gbuffer(gpu, None, cam, res, _smp(), scene=scene)
    assert np.array_equal(bits(gb[..., 10:12]), bits(full[..., 6:8])) and 0 < full[..., 6].sum() < full[..., 7].sum()
    b2, cam2, res2 = LR.point_and_distant(gpu, point=True)
    b1, cam1, res1 = LR.point_and_distant(gpu, point=False)
    _, two, sa = LP.render_lightpass(gpu, b2, cam2, res2, _smp(), lights=[1])
    _, one, sb = LP.render_lightpass(gpu, b1, cam1, res1, _smp())
    assert np.array_equal(bits(two), bits(one)) and sa["rays_any"] == sb["rays_any"] > 0 and 0 < one[..., 0].sum() < one[..., 3].sum()
    from fountain_amd import SceneBuilder, scenes
    b = SceneBuilder(gpu)
    b.material("matte")
    scenes._quad(b, (-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0))
    _, dark, sd = LP.render_lightpass(gpu, b, cam1, res1, _smp())
    assert not dark[..., 0:6].any() and dark[..., 7].sum() >= sd["camera_samples"] and 0 < dark[..., 6].sum() < dark[..., 7].sum()
    assert sd["rays_any"] == 0 and sd["any_launches"] == 0


# ------------------------------------------------------------------ 3. against the oracle's beauty, per sample
def test_matte_beauty_per_sample(gpu, orc_det):
    """All matte (sigma = 0) under a point and a distant light, PathIntegrator(max_depth = 1): the beauty of a sample is its direct term
    from light sampling alone, n_lights * (((Kd * INV_PI) * |cos|) * radiance / pdf) -- five binary32 roundings on Kd, |cos| and the
    radiance --, and the pass's lit is (radiance * (|cos| / pdf)) * n -- three on the same |cos| and radiance.  Kd * INV_PI * lit is formed
    in float64 here, so the two differ by at most 5 + 3 = 8 roundings: 8 * 2^-24 relative.  One sample per call into a zeroed buffer hands
    each sample's own value back (where no other pixel's sample landed)."""
    bound = 8 * U
    rec, film, _ = MR.oracle_records(orc_det, LR.matte_two_lights, PathIntegrator(1, 1.0), _smp())
    L = {(int(r["px"]), int(r["py"]), int(r["sample"])): r["L"] for r in rec}
    b, cam, res = LR.matte_two_lights(gpu)
    scene = b.create_scene()
    from fountain_amd.gbuffer import render_gbuffer
    worst, n_lit, n_dark = 0.0, 0, 0
    for s in range(SPP):
        _, raw, _ = LP.render_lightpass(gpu, None, cam, res, _smp(s, 1), scene=scene)
        gbr, _, _ = render_gbuffer(gpu, None, cam, res, _smp(s, 1), scene=scene)
        alone = (raw[..., 7] == 1.0) & (raw[..., 6] == 1.0)
        assert alone.mean() > 0.5
        for y, x in np.argwhere(alone):
            kd = gbr["albedo"][y, x].astype(np.float64)          # one sample: its albedo itself, Kd
            assert any(np.array_equal(gbr["albedo"][y, x], np.array(v, F32)) for v in LR.KD.values())
            mine = kd * np.float64(LR.INV_PI) * raw[y, x, 0:3].astype(np.float64)
            want = L[(x, y, s)].astype(np.float64)
            assert (np.abs(mine - want) <= bound * np.abs(want)).all(), (x, y, s, mine, want)
            if want.any():
                worst = max(worst, (np.abs(mine - want) / want).max())
            n_lit += bool(want.any()); n_dark += bool(not want.any() and raw[y, x, 3:6].any())
    print("Kd / pi * lit against the oracle's beauty: largest relative difference %.3g (%.2f u, bound 8 u) over %d lit samples; %d in shadow" % (worst, worst / U, n_lit, n_dark))
    assert n_lit > 2000 and n_dark > 50


# ------------------------------------------------------------------ 4. plan independence
def test_crop_splits_tiles_passes_traversal_and_torch(gpu, orc_det, monkeypatch):
    import torch
    name = "every_kind"
    scene, _, _ = _scene(gpu, name)
    res, crop = (33, 17), (0.1, 0.15, 0.93, 0.9)
    from fountain_amd import PerspectiveCamera
    cam = PerspectiveCamera.look_at(gpu, (0.3, -6.0, 3.0), (0.0, 0.0, 0.5), (0, 0, 1), res, fov=40.0)
    kw = dict(scene=scene, crop=crop)
    _, one, st1 = LP.render_lightpass(gpu, None, cam, res, _smp(), **kw)
    assert one.shape[:2] not in ((17, 33),) and st1["rays_any"] > 0 and 0 < one[..., 0].sum() < one[..., 3].sum()
    make = lambda be: (SCENES[name](be)[0], PerspectiveCamera.look_at(be, (0.3, -6.0, 3.0), (0.0, 0.0, 0.5), (0, 0, 1), res, fov=40.0), res)
    ref = LR.replay(orc_det, gpu, make, SPP, SEED, None, crop=crop)
    assert (st1["camera_samples"], st1["rays_any"], st1["spill_samples"]) == (ref["n"], ref["rays_any"], ref["n_spill"])
    LR.assert_matches(one, ref, "33 x 17, unaligned crop")
    own = ref["foreign"] == 0

    def same(other, what):
        assert np.array_equal(bits(other[..., 6:8]), bits(one[..., 6:8])), what
        assert np.array_equal(bits(other[own]), bits(one[own])), what
        assert np.allclose(other, one, rtol=2e-6, atol=1e-6), what

    # a sample range split over two calls into one buffer
    _, two, sa = LP.render_lightpass(gpu, None, cam, res, _smp(0, 1), **kw)
    _, _, sb = LP.render_lightpass(gpu, None, cam, res, _smp(1, SPP - 1), raw=two, **kw)
    same(two, "split sample range")
    assert sa["rays_any"] + sb["rays_any"] == st1["rays_any"] and sa["camera_samples"] + sb["camera_samples"] == st1["camera_samples"]
    # a strided tile range plus its complement
    _, tl, _ = LP.render_lightpass(gpu, None, cam, res, _smp(), tiles=(0, 2, 0), **kw)
    LP.render_lightpass(gpu, None, cam, res, _smp(), tiles=(1, 2, 0), raw=tl, **kw)
    same(tl, "composed tile ranges")
    # one-sample passes
    monkeypatch.setenv("FTN_WF_PATHS_M", "0")
    _, passes, sp = LP.render_lightpass(gpu, None, cam, res, _smp(), **kw)
    monkeypatch.delenv("FTN_WF_PATHS_M")
    assert sp["any_launches"] == SPP and (sp["rays_any"], sp["rays_closest"], sp["spill_samples"]) == (st1["rays_any"], st1["rays_closest"], st1["spill_samples"])
    assert np.array_equal(bits(passes), bits(one))
    # the reference-order walk for the shadow rays
    _, walk, sw = LP.render_lightpass(gpu, None, cam, res, _smp(), count_traffic=1, **kw)
    assert np.array_equal(bits(walk), bits(one)) and sw["rays_any"] == st1["rays_any"]
    # the torch entry, and both stages on the device against their host twins
    film = Film(gpu, res, crop)
    t = torch.zeros((film.height, film.width, 8), dtype=torch.float32, device="cuda:0")
    stt = LP.render_lightpass_torch(scene, cam, film, _smp(), t)
    torch.cuda.synchronize()
    assert stt["rays_any"] == st1["rays_any"]
    same(t.cpu().numpy(), "torch entry")
    assert np.array_equal(bits(t.cpu().numpy()), bits(one))


def test_stages_equal_their_twins(gpu):
    import torch
    from fountain_amd.gbuffer import render_gbuffer
    scene, cam, res = _scene(gpu, "every_kind")
    groups = LP.groups(scene, "kind")
    assert list(groups) == ["point", "distant", "infinite", "area"]
    raws = np.stack([LP.render_lightpass(gpu, None, cam, res, _smp(), lights=idx, scene=scene)[1] for idx in groups.values()])
    t_raw = torch.from_numpy(raws).cuda()
    t_res = torch.empty_like(t_raw)
    LP.resolve_torch(gpu, t_raw, t_res)
    syn = torch.from_numpy(LR.synthetic_sums()).cuda()
    t_syn = torch.empty_like(syn)
    LP.resolve_torch(gpu, syn, t_syn)
    torch.cuda.synchronize()
    res8 = LP.resolve8(gpu, raws)
    assert np.array_equal(bits(t_res.cpu().numpy()), bits(res8)) and np.array_equal(bits(res8), bits(LR.resolve_ref(raws).reshape(res8.shape)))
    assert np.array_equal(bits(t_syn.cpu().numpy()), bits(LR.resolve_ref(LR.synthetic_sums())))
    gb, _, _ = render_gbuffer(gpu, None, cam, res, _smp(), scene=scene)
    gb12 = np.concatenate([gb[k] for k in ("albedo", "normal", "position", "depth", "coverage", "weight")], axis=-1)
    assert gb12.shape[-1] == 12 and (gb12[..., 10] == 0).any() and (gb12[..., 10] != 0).any()
    gains = np.array([[1.0, 0.5, 0.25], [2.0, 2.0, 2.0], [0.0, 1.0, 0.0], [1.5, 1.25, 1.0]], F32)
    t_gb, t_rgb = torch.from_numpy(gb12).cuda(), torch.full(gb12.shape[:2] + (3,), 7.0, dtype=torch.float32, device="cuda:0")
    LP.compose_torch(gpu, t_gb, t_res, gains, t_rgb)
    torch.cuda.synchronize()
    host = LP.compose(gpu, gb12, res8, gains)
    assert np.array_equal(bits(t_rgb.cpu().numpy()), bits(host)) and np.array_equal(bits(host), bits(LR.compose_ref(gb12, res8, gains)))
    assert host.any() and not host[gb12[..., 10] == 0].any()
    # one group of 16 planes through the kernel
    r16 = np.tile(res8[:1], (16, 1, 1, 1))
    g16 = np.linspace(0.1, 1.6, 48, dtype=F32).reshape(16, 3)
    t16 = torch.from_numpy(r16).cuda()
    LP.compose_torch(gpu, t_gb, t16, g16, t_rgb)
    torch.cuda.synchronize()
    assert np.array_equal(bits(t_rgb.cpu().numpy()), bits(LP.compose(gpu, gb12, r16, g16)))


# ------------------------------------------------------------------ 5. refusals with a device
def test_refusals(gpu):
    scene, cam, res = _scene(gpu, "every_kind")
    raw = np.full((24, 40, 8), 3.0, F32)
    for kw, code in ((dict(lights=[]), A.FTN_ERR_INVALID_ARGUMENT), (dict(lights=[1, 1]), A.FTN_ERR_INVALID_ARGUMENT), (dict(lights=[2, 1]), A.FTN_ERR_INVALID_ARGUMENT),
                     (dict(lights=[0, 5]), A.FTN_ERR_INVALID_ARGUMENT), (dict(lights=[5]), A.FTN_ERR_INVALID_ARGUMENT),
                     (dict(pipeline=A.FTN_PIPELINE_MEGAKERNEL), A.FTN_ERR_UNSUPPORTED), (dict(lights=[7], pipeline=A.FTN_PIPELINE_MEGAKERNEL), A.FTN_ERR_INVALID_ARGUMENT)):
        with pytest.raises(FountainError) as e:
            LP.render_lightpass(gpu, None, cam, res, _smp(), scene=scene, raw=raw, **kw)
        assert e.value.code == code, kw
    with pytest.raises(FountainError) as e:
        LP.render_lightpass(gpu, None, cam, res, RandomSampler(2, 5, indexed=False), scene=scene, raw=raw)
    assert e.value.code == A.FTN_ERR_UNSUPPORTED
    with pytest.raises(FountainError) as e:
        LP.render_lightpass(gpu, None, cam, res, RandomSampler(2, 5, indexed=False), lights=[9], scene=scene, raw=raw)
    assert e.value.code == A.FTN_ERR_INVALID_ARGUMENT
    assert (raw == 3.0).all()
    _, ok, _ = LP.render_lightpass(gpu, None, cam, res, _smp(), lights=[4], scene=scene)
    assert ok[..., 3:6].any()


# ------------------------------------------------------------------ 6. CLI
def test_cli_writes_the_groups_and_relight_reproduces_compose(gpu, tmp_path):
    from fountain_amd import render
    from fountain_amd.api import PbrtScene, read_exr
    from fountain_amd.gbuffer import render_gbuffer
    scene_file = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "cornell.pbrt")
    out = str(tmp_path / "out.exr")
    assert render.main([scene_file, "-o", out, "--samples", "2", "--light-groups", "--gbuffer"]) == 0
    parsed = PbrtScene(scene_file, gpu)
    scene = parsed.create_scene()
    groups = LP.groups(scene, "kind")
    assert groups and os.path.exists(out)
    smp = parsed.sampler(2, indexed=True)
    res8 = []
    for name, idx in groups.items():
        want, raw, _ = LP.render_lightpass(gpu, None, parsed.camera, None, smp, lights=idx, scene=scene, film=parsed.film())
        paths = render.lightpass_paths(out, name)
        assert np.array_equal(bits(read_exr(paths["light"], gpu)), bits(want["lit"]))
        assert np.array_equal(bits(read_exr(paths["lightvis"], gpu)), bits(np.repeat(want["visibility"], 3, axis=-1)))
        assert want["lit"].any() and want["visibility"].min() < 1 and (want["visibility"] >= 0).all()
        res8.append(LP.resolve8(gpu, raw))
    assert sorted(p for p in os.listdir(tmp_path) if "_light" in p) == sorted(os.path.basename(v) for n in groups for v in render.lightpass_paths(out, n).values())
    # the same command without the flag writes the same image
    plain = str(tmp_path / "plain.exr")
    assert render.main([scene_file, "-o", plain, "--samples", "2"]) == 0
    assert open(plain, "rb").read() == open(out, "rb").read()
    # relight with gains of 1 on the written files reproduces compose
    gb, _, _ = render_gbuffer(gpu, None, parsed.camera, None, smp, scene=scene, film=parsed.film())
    gb12 = np.concatenate([gb[k] for k in ("albedo", "normal", "position", "depth", "coverage", "weight")], axis=-1)
    relit = str(tmp_path / "relit.exr")
    argv = ["relight", "--albedo", render.gbuffer_paths(out)["albedo"], "-o", relit]
    for name in groups:
        argv += ["--light", "%s=%s:1,1,1" % (name, render.lightpass_paths(out, name)["light"])]
    assert LP.main(argv) == 0
    want = LP.compose(gpu, gb12, np.stack(res8), np.ones((len(groups), 3), F32))
    assert np.array_equal(bits(read_exr(relit, gpu)), bits(want)) and want.any()
