"""Per-pixel second moments on the GPU (include/fountain_hip_moments.h, fountain_amd/moments.py): the beauty is ftn_render's; the Y
moment equals a float32 sum rebuilt from single-sample ftn_render films, bit for bit; a constant-radiance scene with spill gives the
closed form of every accumulator; chunks, sample-range splits and the device path; the variance estimate against the spread of the
means over many seeds; refusals; a config-5-sized scene; the CLI."""
import ctypes as C
import os

import numpy as np
import pytest

from fountain_amd import (DirectLightingIntegrator, FountainError, PathIntegrator, PerspectiveCamera, RandomSampler, SamplerIntegrator,
                          SceneBuilder, WhittedIntegrator, scenes, _abi as A)
from fountain_amd import moments as M

import _gbuffer_ref as GR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO, MEGA, WAVE = A.FTN_PIPELINE_AUTO, A.FTN_PIPELINE_MEGAKERNEL, A.FTN_PIPELINE_WAVEFRONT
F32 = np.float32
bits = GR.bits
TIMES = ("kernel_ms", "trace_ms", "any_ms", "shade_ms", "sort_ms")


def counters(st):
    return {k: v for k, v in st.items() if k not in TIMES}


def xyz_to_rgb(xyz):
    """ftn_math.h's xyz_to_rgb in float32, left to right"""
    x, y, z = (xyz[..., k].astype(F32) for k in range(3))
    return np.stack([F32(3.240479) * x - F32(1.537150) * y - F32(0.498535) * z,
                     F32(-0.969256) * x + F32(1.875991) * y + F32(0.041556) * z,
                     F32(0.055648) * x - F32(0.204043) * y + F32(1.057311) * z], -1).astype(F32)


def beauty(be, scene, cam, film, integ, smp, tiles=None, pipeline=AUTO):
    st = SamplerIntegrator(cam, integ).render_parallel(scene, film, smp, tiles=tiles, pipeline=pipeline)
    return film.pixels, st


def textured_env(be, res=40):
    """a checkerboard floor and a matte sphere under the procedural sky (an image environment light)"""
    b = SceneBuilder(be)
    b.light_source("infinite", texels=scenes.sky_envmap(64))
    b.texture("chk", "spectrum", "checkerboard", uscale=8.0, vscale=8.0, tex1=(0.7, 0.7, 0.7), tex2=(0.2, 0.3, 0.45))
    b.material("matte", Kd="chk")
    scenes._quad(b, (-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0))
    b.attribute_begin(); b.material("plastic", Kd=(0.3, 0.1, 0.1), Ks=(0.4, 0.4, 0.4), roughness=0.05); b.translate((0, 0, 0.6)); b.shape("sphere", radius=0.6); b.attribute_end()
    cam = PerspectiveCamera.look_at(be, (0.5, -3.5, 1.8), (0, 0, 0.4), (0, 0, 1), (res, res), fov=50.0)
    return b, cam, (res, res)


def constant_sphere(be, res=24, L=(0.7, 1.3, 2.1)):
    """the camera inside a black-matte emitting sphere: every camera sample returns L (Le, then nothing to reflect)"""
    b = SceneBuilder(be)
    b.attribute_begin()
    b.material("matte", Kd=(0.0, 0.0, 0.0))
    b.area_light_source("diffuse", L=L)
    b.reverse_orientation()
    b.shape("sphere", radius=50.0)
    b.attribute_end()
    cam = PerspectiveCamera.look_at(be, (0, -2, 0), (0, 0, 0), (0, 0, 1), (res, res), fov=60.0)
    return b, cam, (res, res)


# ------------------------------------------------------------------ 1. the beauty is ftn_render's
CASES = [("cornell", "path", (0.5, 0.5), (0.0, 0.0, 1.0, 1.0), None),
         ("cornell", "path", (1.25, 1.25), (0.1, 0.05, 0.9, 0.95), (1, 2, 0)),
         ("cornell", "direct", (0.5, 0.5), (0.0, 0.0, 1.0, 1.0), None),
         ("cornell", "whitted", (1.25, 1.25), (0.0, 0.0, 1.0, 1.0), None),
         ("env", "path", (0.5, 0.5), (0.0, 0.0, 1.0, 1.0), (0, 2, 0)),
         ("env", "path", (1.25, 1.25), (0.2, 0.0, 1.0, 0.8), None),
         ("env", "direct", (0.5, 0.5), (0.0, 0.0, 1.0, 1.0), None)]


@pytest.mark.parametrize("which,integ,radius,crop,tiles", CASES)
def test_beauty_is_ftn_render(gpu, which, integ, radius, crop, tiles):
    """pixels, statistics and return code of ftn_render for the same arguments.  The weights are integer sums and equal everywhere; the
    values are equal bit for bit on every pixel that no other pixel's sample reached.  The others are summed by atomics in the order the
    GPU runs them, so two identical ftn_render calls can already differ there in the last bits."""
    b, cam, res = scenes.cornell(gpu, res=40) if which == "cornell" else textured_env(gpu)
    integrator = {"path": PathIntegrator(5, 1.0), "direct": DirectLightingIntegrator(4), "whitted": WhittedIntegrator(4)}[integ]
    smp = RandomSampler(4, 17, indexed=True)
    scene = b.create_scene()
    want, st_want = beauty(gpu, scene, cam, GR.film(gpu, res, crop, radius), integrator, smp, tiles)
    var, film, mom, st = M.render_moments(gpu, None, cam, res, integrator, smp, tiles=tiles, scene=scene, film=GR.film(gpu, res, crop, radius))
    assert counters(st) == counters(st_want)
    assert st["camera_samples"] > 0 and (radius[0] == 0.5) == (st["spill_samples"] < 8)
    got = film.pixels
    assert np.array_equal(bits(got[..., 3]), bits(want[..., 3]))
    if radius[0] == 0.5:                                             # (with radius 1.25 every pixel receives other pixels' samples)
        own = got[..., 3] == 4                                       # weight = spp: nothing foreign landed here
        assert own.sum() > 0.99 * (got[..., 3] > 0).sum()
        assert np.array_equal(bits(got[own]), bits(want[own]))
    assert np.allclose(got, want, rtol=1e-5, atol=1e-6)
    assert np.isfinite(mom).all() and (mom >= 0).all() and (mom[got[..., 3] > 0].sum(-1) > 0).any()


# ------------------------------------------------------------------ 2. the Y moment from single-sample films
def single_sample_films(gpu, scene, cam, res, integ, spp, seed, radius=(0.5, 0.5)):
    """ftn_render over [s, s + 1) into a zero film, for every s: with radius 0.5 xyz[1] is that sample's Y (0 + Y, then 0 + that)"""
    out = []
    for s in range(spp):
        px, _ = beauty(gpu, scene, cam, GR.film(gpu, res, radius=radius), integ, RandomSampler(spp, seed, indexed=True, first_sample=s, sample_count=1))
        out.append(px.copy())
    return np.stack(out)


def test_y_moment_from_single_sample_films(gpu):
    spp, seed = 6, 3
    b, cam, res = scenes.cornell(gpu, res=32)
    scene = b.create_scene()
    integ = PathIntegrator(5, 1.0)
    films = single_sample_films(gpu, scene, cam, res, integ, spp, seed)
    _, film, mom, st = M.render_moments(gpu, None, cam, res, integ, RandomSampler(spp, seed, indexed=True), scene=scene)
    own = film.pixels[..., 3] == spp                                  # no sample of another pixel landed here
    assert own.mean() > 0.99
    y = films[..., 1]
    want = np.zeros(y.shape[1:], F32)
    for s in range(spp):                                              # float32, from +0, in sample order
        want = (want + (y[s] * y[s]).astype(F32)).astype(F32)
    assert np.array_equal(bits(mom[..., 3][own]), bits(want[own]))
    rgb = xyz_to_rgb(films[..., :3]).astype(np.float64)
    sq = (rgb * rgb).sum(0)
    assert np.allclose(mom[..., :3][own], sq[own], rtol=1e-5, atol=1e-6 * sq.max())
    assert (mom[..., 3][own] > 0).mean() > 0.5


# ------------------------------------------------------------------ 3. closed form with spill
def seq_sum(v, n):
    """float32 sum of n copies of v, one addition at a time from +0 (any order gives these bits: every addend is the same)"""
    table = [F32(0)]
    for _ in range(int(n.max()) if n.size else 0):
        table.append(F32(table[-1] + v))
    return np.array(table, F32)[n]


def test_closed_form_with_spill(gpu, orc_det):
    spp, seed, radius = 3, 21, (1.25, 1.25)
    L = (0.7, 1.3, 2.1)
    b, cam, res = constant_sphere(gpu)
    scene = b.create_scene()
    integ = PathIntegrator(5, 1.0)
    films = single_sample_films(gpu, scene, cam, res, integ, spp, seed)
    c = np.array(L, F32)
    xyz_c = np.array([(F32(0.412453) * c[0] + F32(0.357580) * c[1]) + F32(0.180423) * c[2],
                      (F32(0.212671) * c[0] + F32(0.715160) * c[1]) + F32(0.072169) * c[2],
                      (F32(0.019334) * c[0] + F32(0.119193) * c[1]) + F32(0.950227) * c[2]], F32)
    # every sample returns c, bit for bit: each single-sample film holds rgb_to_xyz(c) on every pixel its own sample reached alone
    hit = films[..., 3] == 1
    assert hit.mean() > 0.99 and np.array_equal(bits(films[..., :3][hit]), bits(np.broadcast_to(xyz_c, films[..., :3][hit].shape)))
    Y = xyz_c[1]
    _, film, mom, st = M.render_moments(gpu, None, cam, res, integ, RandomSampler(spp, seed, indexed=True), scene=scene,
                                        film=GR.film(gpu, res, radius=radius))
    # the own, in-tile and other-tile counts from the footprints of the oracle's sample positions
    f = GR.film(orc_det, res, radius=radius)
    cr = f.desc.crop
    n = np.zeros((3,) + film.pixels.shape[:2], np.int64)
    n_spill = 0
    u5 = (C.c_float * 5)()
    for tile in GR.selected_tiles(f, None):
        tpb = GR.tile_pixel_bounds(f, tile)
        for py in range(tile[1], tile[3]):
            for px in range(tile[0], tile[2]):
                for s in range(spp):
                    orc_det.lib.orc_kat_indexed_f32(C.c_uint64(seed), C.c_int32(px), C.c_int32(py), C.c_uint32(s), u5, C.c_size_t(5))
                    touched = GR.footprint(f, tpb, F32(px) + F32(u5[0]), F32(py) + F32(u5[1]))
                    n_spill += len(touched) != 1
                    for (x, y) in touched:
                        k = 0 if (x, y) == (px, py) else 1 if tile[0] <= x < tile[2] and tile[1] <= y < tile[3] else 2
                        n[k, y - cr[1], x - cr[0]] += 1
    assert np.array_equal(film.pixels[..., 3], n.sum(0).astype(F32))
    assert st["spill_samples"] == n_spill and n[1].any() and n[2].any()
    want = np.zeros(mom.shape, F32)
    for ch, v in enumerate([c[0] * c[0], c[1] * c[1], c[2] * c[2], Y * Y]):
        a, bb, cc = (seq_sum(F32(v), n[k]) for k in range(3))
        want[..., ch] = ((F32(0) + (a + bb).astype(F32)) + cc).astype(F32)
    assert np.array_equal(bits(mom), bits(want))
    var = M.resolve(gpu, film.pixels, mom)
    assert (np.abs(var[..., :3]) <= 1e-6 * c * c).all() and (np.abs(var[..., 3]) <= 1e-6 * Y * Y).all()


# ------------------------------------------------------------------ 4. chunks, splits, the device path
def test_chunks_splits_and_device_path(gpu, monkeypatch):
    """FTN_WF_PATHS_M=1 on a 256^2 film: chunks of 16 samples, 37 spp as 16 + 16 + 5, equal to one chunk bit for bit; a split sample
    range added into one buffer equals the sum of the two calls' own results; the device path adds into what the tensors hold"""
    import torch
    spp, seed = 37, 8
    b, cam, res = scenes.cornell(gpu, res=256)
    scene = b.create_scene()
    integ = PathIntegrator(5, 1.0)
    smp = RandomSampler(spp, seed, indexed=True)
    _, one, m_one, st1 = M.render_moments(gpu, None, cam, res, integ, smp, scene=scene)
    one = one.pixels
    px_r, st_r = beauty(gpu, scene, cam, GR.film(gpu, res), integ, smp)
    assert np.array_equal(bits(one), bits(px_r)) and counters(st1) == counters(st_r)
    monkeypatch.setenv("FTN_WF_PATHS_M", "1")
    _, many, m_many, st = M.render_moments(gpu, None, cam, res, integ, smp, scene=scene)
    px_r2, st_r2 = beauty(gpu, scene, cam, GR.film(gpu, res), integ, smp)
    assert counters(st) == counters(st_r2) and st["trace_launches"] > st1["trace_launches"]
    assert np.array_equal(bits(many.pixels), bits(one)) and np.array_equal(bits(m_many), bits(m_one))
    monkeypatch.delenv("FTN_WF_PATHS_M")
    for k in (5, 16):
        parts = [M.render_moments(gpu, None, cam, res, integ, RandomSampler(spp, seed, indexed=True, first_sample=a, sample_count=n), scene=scene)
                 for a, n in ((0, k), (k, spp - k))]
        _, split, m_split, _ = M.render_moments(gpu, None, cam, res, integ, RandomSampler(spp, seed, indexed=True, first_sample=0, sample_count=k), scene=scene)
        M.render_moments(gpu, None, cam, res, integ, RandomSampler(spp, seed, indexed=True, first_sample=k, sample_count=spp - k), scene=scene,
                         film=split, moments=m_split)
        assert np.array_equal(bits(split.pixels), bits((parts[0][1].pixels + parts[1][1].pixels).astype(F32))), k
        assert np.array_equal(bits(m_split), bits((parts[0][2] + parts[1][2]).astype(F32))), k
        assert np.allclose(m_split, m_one, rtol=1e-5, atol=1e-6), k
    # device path, added into existing contents (host: the call's sums from zero, then added; device: added in k_film_resolve's order,
    # the same bits wherever no sample of another tile landed)
    rng = np.random.default_rng(1)
    e_px, e_m = rng.uniform(0, 3, one.shape).astype(F32), rng.uniform(0, 3, one.shape).astype(F32)
    film = GR.film(gpu, res)
    film.pixels[...] = e_px
    _, film, m_host, _ = M.render_moments(gpu, None, cam, res, integ, smp, scene=scene, film=film, moments=e_m.copy())
    t_px, t_m = torch.from_numpy(e_px).cuda(), torch.from_numpy(e_m).cuda()
    st_d = M.render_moments_torch(scene, cam, GR.film(gpu, res), integ, smp, t_px, t_m)
    torch.cuda.synchronize()
    assert counters(st_d) == counters(st1)
    own = one[..., 3] == spp
    d_px, d_m = t_px.cpu().numpy(), t_m.cpu().numpy()
    assert np.array_equal(bits(d_px[own]), bits(film.pixels[own])) and np.array_equal(bits(d_m[own]), bits(m_host[own]))
    assert np.allclose(d_m, m_host, rtol=1e-6, atol=1e-6) and np.allclose(d_px, film.pixels, rtol=1e-6, atol=1e-6)
    # and the device resolve equals the host's bit for bit
    out = torch.empty_like(t_px)
    M.resolve_torch(gpu, torch.from_numpy(one).cuda(), torch.from_numpy(m_one).cuda(), out)
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(M.resolve(gpu, one, m_one)))


@pytest.mark.parametrize("integ_cls", [DirectLightingIntegrator, WhittedIntegrator])
def test_chunks_direct_lighting_and_whitted(gpu, monkeypatch, integ_cls):
    """the direct-lighting / Whitted branch of the pass plan through the moments driver: FTN_WF_PATHS_M=1 on a 256^2 film gives passes
    of 16 samples (2^20 paths / 65,536 slots), 20 spp as 16 + 4, equal to one pass and to ftn_render bit for bit"""
    spp, seed = 20, 8
    b, cam, res = scenes.cornell(gpu, res=256)
    scene = b.create_scene()
    integ = integ_cls(4)
    smp = RandomSampler(spp, seed, indexed=True)
    _, one, m_one, st1 = M.render_moments(gpu, None, cam, res, integ, smp, scene=scene)
    px_r, st_r = beauty(gpu, scene, cam, GR.film(gpu, res), integ, smp)
    assert np.array_equal(bits(one.pixels), bits(px_r)) and counters(st1) == counters(st_r)
    monkeypatch.setenv("FTN_WF_PATHS_M", "1")
    _, many, m_many, st = M.render_moments(gpu, None, cam, res, integ, smp, scene=scene)
    px_r2, st_r2 = beauty(gpu, scene, cam, GR.film(gpu, res), integ, smp)
    assert np.array_equal(bits(many.pixels), bits(px_r2)) and counters(st) == counters(st_r2)
    assert st["trace_launches"] > st1["trace_launches"]
    assert np.array_equal(bits(many.pixels), bits(one.pixels)) and np.array_equal(bits(m_many), bits(m_one))


# ------------------------------------------------------------------ 5. statistics
def test_variance_matches_the_spread_of_the_means(gpu):
    """Cornell, 32^2, 8 spp, 48 seeds: the mean predicted variance of the Y mean, summed over the pixels, against the variance of the Y
    means across seeds.  The bound [0.75, 1.33] was set before measuring; the first GPU run observed a ratio of 0.98."""
    spp, n_seeds = 8, 48
    b, cam, res = scenes.cornell(gpu, res=32)
    scene = b.create_scene()
    integ = PathIntegrator(5, 1.0)
    means, preds = [], []
    for seed in range(n_seeds):
        var, film, mom, _ = M.render_moments(gpu, None, cam, res, integ, RandomSampler(spp, 1000 + seed, indexed=True), scene=scene)
        w = film.pixels[..., 3]
        assert (w >= 2).all()
        means.append(film.pixels[..., 1].astype(np.float64) / w)
        preds.append(var[..., 3].astype(np.float64))
    means, preds = np.stack(means), np.stack(preds)
    empirical = means.var(0, ddof=1).sum()
    predicted = preds.mean(0).sum()
    ratio = predicted / empirical
    print("predicted / empirical variance of the Y means: %.4f" % ratio)
    assert 0.75 <= ratio <= 1.33, ratio


# ------------------------------------------------------------------ 6. refusals on the device
def test_refusals(gpu):
    b, cam, res = scenes.cornell(gpu, res=16)
    scene = b.create_scene()
    integ = PathIntegrator(3, 1.0)
    for kw in (dict(sampler=RandomSampler(2, 0)), dict(pipeline=MEGA)):
        with pytest.raises(FountainError) as e:
            M.render_moments(gpu, None, cam, res, integ, kw.get("sampler", RandomSampler(2, 0, indexed=True)), scene=scene, pipeline=kw.get("pipeline", AUTO))
        assert e.value.code == A.FTN_ERR_UNSUPPORTED

    def many_lights(be, n):
        bb, c, r = scenes.cornell(be, res=16)
        for k in range(n):
            bb.light_source("point", I=(1 + 0.1 * k, 1, 1), from_=(0.07 * k - 0.5, 0.03 * k, 0.5))
        return bb, c, r
    n_area = len(many_lights(gpu, 0)[0].create_scene().lights()[0])
    smp = RandomSampler(2, 0, indexed=True)
    for pl in (AUTO, WAVE):
        bb, c, r = many_lights(gpu, 33 - n_area)
        with pytest.raises(FountainError) as e:
            M.render_moments(gpu, bb, c, r, WhittedIntegrator(3), smp, pipeline=pl)
        assert e.value.code == A.FTN_ERR_UNSUPPORTED
    bb, c, r = many_lights(gpu, 32 - n_area)                            # exactly 32 lights: accepted, the beauty is ftn_render's
    sc = bb.create_scene()
    _, film, _, _ = M.render_moments(gpu, None, c, r, WhittedIntegrator(3), smp, scene=sc)
    assert np.array_equal(bits(film.pixels), bits(beauty(gpu, sc, c, GR.film(gpu, r), WhittedIntegrator(3), smp)[0]))
    # NaN radiance: the code of ftn_render (a second, NaN-valued emitter on the back wall of the Cornell box)
    nb, ncam, nres = scenes.cornell(gpu, res=16)
    nb.attribute_begin(); nb.material("matte", Kd=(0.0, 0.0, 0.0)); nb.area_light_source("diffuse", L=(float("nan"), 1.0, 1.0))
    scenes._quad(nb, (-0.2, 0.99, -0.2), (0.2, 0.99, -0.2), (0.2, 0.99, 0.2), (-0.2, 0.99, 0.2)); nb.attribute_end()
    nscene = nb.create_scene()
    with pytest.raises(FountainError) as e_r:
        beauty(gpu, nscene, ncam, GR.film(gpu, nres), integ, smp)
    with pytest.raises(FountainError) as e_m:
        M.render_moments(gpu, None, ncam, nres, integ, smp, scene=nscene)
    assert e_m.value.code == e_r.value.code == A.FTN_ERR_NAN_RADIANCE


# ------------------------------------------------------------------ 7. scale
def test_config5_scene_at_4096(gpu, monkeypatch):
    """the config-5-sized scene at 4096^2, 2 spp: the beauty is ftn_render's, and two chunks (FTN_WF_PATHS_M=16: one sample each) give
    the moments of one.  A pixel that received three or more samples of other pixels in one spill sum may be summed in another order
    (weight above spp + 2); it is compared within rounding."""
    spp = 2
    b, cam, res = scenes.instanced_cubes(gpu, res=(4096, 4096))
    scene = b.create_scene()
    integ = PathIntegrator(5, 1.0)
    smp = RandomSampler(spp, 5, indexed=True)
    _, one, m_one, st = M.render_moments(gpu, None, cam, res, integ, smp, scene=scene)
    assert st["camera_samples"] == spp * 4096 * 4096
    px_r, st_r = beauty(gpu, scene, cam, GR.film(gpu, res), integ, smp)
    assert counters(st) == counters(st_r)
    sure = one.pixels[..., 3] <= spp + 2
    assert sure.mean() > 0.999
    assert np.array_equal(bits(one.pixels[..., 3]), bits(px_r[..., 3]))
    assert np.array_equal(bits(one.pixels[sure]), bits(px_r[sure])) and np.allclose(one.pixels, px_r, rtol=1e-5, atol=1e-6)
    monkeypatch.setenv("FTN_WF_PATHS_M", "16")
    _, two, m_two, st2 = M.render_moments(gpu, None, cam, res, integ, smp, scene=scene)
    monkeypatch.delenv("FTN_WF_PATHS_M")
    assert st2["trace_launches"] > st["trace_launches"] and st2["camera_samples"] == st["camera_samples"]
    assert np.array_equal(bits(m_two[sure]), bits(m_one[sure])) and np.allclose(m_two, m_one, rtol=1e-5, atol=1e-6)
    assert np.array_equal(bits(two.pixels[sure]), bits(one.pixels[sure]))
    assert np.isfinite(m_one).all() and (m_one >= 0).all()


# ------------------------------------------------------------------ 8. CLI
def test_cli_writes_the_variance(gpu, tmp_path):
    from fountain_amd import render
    from fountain_amd.api import PbrtScene, read_exr
    scene_file = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    plain, with_var, all_three = str(tmp_path / "plain.exr"), str(tmp_path / "var.exr"), str(tmp_path / "all.exr")
    assert render.main([scene_file, "-o", plain, "--samples", "4"]) == 0
    assert render.main([scene_file, "-o", with_var, "--samples", "4", "--variance"]) == 0
    assert open(plain, "rb").read() == open(with_var, "rb").read()
    parsed = PbrtScene(scene_file, gpu)
    film = parsed.film()
    var, _, _, _ = M.render_moments(gpu, None, parsed.camera, None, PathIntegrator(5, 1.0), parsed.sampler(4, indexed=True),
                                    scene=parsed.create_scene(), film=film)
    assert np.array_equal(bits(read_exr(render.variance_path(with_var), gpu)), bits(var[..., :3]))
    assert render.main([scene_file, "-o", all_three, "--samples", "4", "--variance", "--gbuffer", "--denoise"]) == 0
    assert open(plain, "rb").read() == open(all_three, "rb").read()
    for p in [render.variance_path(all_three), render.denoised_path(all_three)] + list(render.gbuffer_paths(all_three).values()):
        assert os.path.exists(p), p
    assert np.array_equal(bits(read_exr(render.variance_path(all_three), gpu)), bits(var[..., :3]))
    assert render.main([scene_file, "-o", str(tmp_path / "x.exr"), "--variance", "--exact-stream"]) == 2
    assert render.main([scene_file, "-o", str(tmp_path / "x.exr"), "--variance", "--gpus", "2"]) == 2
